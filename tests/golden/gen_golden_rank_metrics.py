"""Records tests/golden/rank_metrics_*.json / .npz: inputs in the reference's own form (string ids, qrels and candidate
dicts, scores in arrival order) and what the REAL functions of matchmaker/utils/core_metrics.py return for them.

    python tests/golden/gen_golden_rank_metrics.py            (needs the reference tree: oracle/ref_harness.REFERENCE_ROOT)

The tests read only the recorded files.  Non-default cutoffs are recorded by assigning the module's global_metric_config
before the calls, which is how a user of the reference changes them.
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_harness as R      # noqa: E402

DEFAULT = {"MRR+Recall@": [10, 20, 100, 200, 1000], "nDCG@": [3, 5, 10, 20, 1000], "MAP@": 1000}


def load_core_metrics():
    spec = importlib.util.spec_from_file_location("ref_core_metrics",
                                                  os.path.join(R.REFERENCE_ROOT, "matchmaker", "utils", "core_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Case:
    def __init__(self, name, config, binarization_point):
        self.name, self.config, self.binp = name, config, binarization_point
        self.qids, self.dids, self.scores, self.qrels, self.cand = [], [], [], {}, {}

    def add(self, qid, docs, scores, judged=None, cand_order=None):
        """docs in ARRIVAL order with their scores; cand_order: the first-stage ranking (doc ids), default arrival order."""
        assert len(docs) == len(scores)
        self.qids += [qid] * len(docs)
        self.dids += list(docs)
        self.scores += [float(np.float32(s)) for s in scores]
        if judged is not None:
            self.qrels[qid] = dict(judged)
        uniq = list(dict.fromkeys(docs if cand_order is None else cand_order))
        self.cand[qid] = {d: i + 1 for i, d in enumerate(uniq)}


def descending(n):
    return [float(n - i) for i in range(n)]


def case_edges():
    """Default cutoffs, binarization point 1: the cutoff edges, grade-0 and all-zero judgements, a truncated idcg, a query
    outside the qrels, duplicate doc ids; ties keep arrival order."""
    c = Case("edges", DEFAULT, 1.0)
    docs = lambda q, n: [f"{q}_d{i}" for i in range(n)]
    c.add("none", docs("none", 12), descending(12), {"elsewhere": 1})
    for r in (1, 10, 11):
        d = docs(f"r{r}", 15)
        c.add(f"r{r}", d, descending(15), {d[r - 1]: 1})
    for r in (1000, 1001):                                       # MAP@1000 / Recall@1000 edge: a 1001-row list
        d = docs(f"r{r}", 1001)
        c.add(f"r{r}", d, descending(1001), {d[r - 1]: 1, d[4]: 0}, cand_order=d[::-1])
    d = docs("g0", 8)
    c.add("g0", d, descending(8), {d[0]: 0, d[3]: 1})            # judged grade 0: in nDCG's mask, not binary-relevant
    d = docs("all0", 6)
    c.add("all0", d, descending(6), {d[1]: 0, d[2]: 0})          # every judged grade 0: nDCG = 0 / 0
    d = docs("many", 30)
    c.add("many", d, descending(30), {d[i]: 1 + i % 3 for i in range(0, 30, 3)}, cand_order=d[15:] + d[:15])
    c.add("unjudged", docs("unjudged", 5), descending(5), None)  # not in the qrels
    d = docs("dup", 6)
    c.add("dup", [d[0], d[1], d[1], d[2], d[1], d[3]], [3.0, 2.0, 2.0, 2.0, 1.0, 0.5], {d[1]: 2, d[3]: 1})
    d = docs("ties", 9)
    c.add("ties", d, [1.0, 2.0, 1.0, 2.0, 0.0, -0.0, 2.0, 1.0, 0.0], {d[2]: 1, d[5]: 1, d[8]: 3}, cand_order=d[::-1])
    d = docs("zero_four", 6)                                     # thresholds 1..2 drop the first relevant row, keep the later one
    c.add("zero_four", d, descending(6), {d[0]: 1, d[3]: 1}, cand_order=[d[3], d[5], d[0], d[1], d[2], d[4]])
    return c, {"single": [1, 2, 5, 10, 11, 500, 1000, 1001], "depth": []}


def case_graded(seed=5):
    """Grades 0-3 with binarization point 2, non-default cutoffs, 40 lists of 1 .. 65 rows, scores from 5 values, first-stage
    ranks unrelated to the model order."""
    rng = np.random.default_rng(seed)
    c = Case("graded", {"MRR+Recall@": [1, 3, 7], "nDCG@": [2, 4], "MAP@": 5}, 2.0)
    for q in range(40):
        n = [1, 2, 63, 64, 65][q] if q < 5 else int(rng.integers(1, 66))
        pool = [f"d{int(x)}" for x in rng.permutation(90)]
        docs = pool[:n]
        if q % 6 == 1 and n > 3:
            docs[2] = docs[0]
        judged = None
        if q % 9 != 4:
            judged = {str(d): int(rng.integers(0, 4)) for d in rng.permutation(pool[:max(n, 12)])[:int(rng.integers(1, 9))]}
            if q % 8 == 3:
                judged = {d: 0 for d in judged}
        uniq = list(dict.fromkeys(docs))
        c.add(f"q{q}", docs, rng.integers(0, 5, n).astype(np.float32) / 2 - 1, judged,
              cand_order=[uniq[int(i)] for i in rng.permutation(len(uniq))])
    return c, {"single": [1, 2, 3, 7, 33, 65], "depth": [(1, 65), (65, 65), (1, 100)]}


def case_short(hi, seed):
    rng = np.random.default_rng(seed)
    c = Case(f"short{hi}", {"MRR+Recall@": [1, 2, 5], "nDCG@": [1, 3], "MAP@": 4}, 1.0)
    for q in range(9):
        n = hi if q == 0 else int(rng.integers(1, hi + 1))
        docs = [f"d{int(x)}" for x in rng.permutation(3 * hi + 6)[:n]]
        judged = {d: int(rng.integers(0, 3)) for d in docs[:int(rng.integers(1, 3))]} if q != 5 else None
        c.add(f"q{q}", docs, rng.integers(0, 3, n).astype(np.float32), judged,
              cand_order=[docs[int(i)] for i in rng.permutation(n)])
    return c, {"single": [1, hi], "depth": [(1, hi), (hi, hi)]}


def record(cm, case, plan):
    cm.global_metric_config = case.config
    unrolled = {}
    for q, d, s in zip(case.qids, case.dids, case.scores):
        unrolled.setdefault(q, []).append((d, s))
    ranking = cm.unrolled_to_ranked_result(unrolled)
    arrays = {"scores": np.array(case.scores, np.float32)}

    def keep(tag, out):
        d, rr, ap, rec, ndcg = out
        arrays.update({tag + "_rr": rr, tag + "_ap": ap, tag + "_recall": rec, tag + "_ndcg": ndcg})
        return {k: float(v) for k, v in d.items()}

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        js = {"name": case.name, "config": case.config, "binarization_point": case.binp, "query_ids": case.qids,
              "doc_ids": case.dids, "qrels": case.qrels, "candidate_ranking": case.cand, "ranking": ranking,
              "plain": keep("plain", cm.calculate_metrics_plain(ranking, case.qrels, case.binp, return_per_query=True)),
              "single": {}, "depth": []}
        for t in plan["single"]:
            js["single"][str(t)] = keep(f"single{t}", cm.calculate_metrics_single_candidate_threshold(
                ranking, case.qrels, case.cand, t, case.binp, return_per_query=True))
        for lo, hi in plan["depth"]:
            res = cm.calculate_metrics_along_candidate_depth(ranking, case.qrels, case.cand, (lo, hi), case.binp)
            keys = list(res[lo])
            js["depth"].append({"range": [lo, hi], "keys": keys})
            arrays[f"depth_{lo}_{hi}"] = np.array([[float(res[t][k]) for k in keys] for t in range(lo, hi + 1)])
    with open(os.path.join(HERE, f"rank_metrics_{case.name}.json"), "w") as f:
        json.dump(js, f)
    np.savez_compressed(os.path.join(HERE, f"rank_metrics_{case.name}.npz"), **arrays)


if __name__ == "__main__":
    cm = load_core_metrics()
    for case, plan in (case_edges(), case_graded(), case_short(1, 11), case_short(7, 12), case_short(64, 13)):
        record(cm, case, plan)
        print("recorded", case.name)
