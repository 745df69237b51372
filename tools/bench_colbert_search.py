#!/usr/bin/env python
"""Benchmark of ColBERT end-to-end retrieval (TokenStore.search_device) on one GPU: a synthetic store of MSMARCO-length
passages (the generator of bench.py's ragged-aggregate leg: lengths N(70, 25) clipped to [8, 180], unit fp16 token
vectors, dim 128), nq in {1, 64} queries of Q 32 tokens, k' in {128, 512} token hits per query token, top_n 1000.
Prints ONE JSON line; per (nq, k'):

  token_search_ms, candidates_ms, maxsim_ms, selection_ms
                     the four stages, median of per-call HIP events in steady state (bench.gpu_time_ms): ops.dot_topk over the
                     whole token matrix, ops.colbert_candidates, ops.maxsim_ragged over the trimmed candidate slots,
                     -inf fill + ops.topk_merge
  rank_hits_ms       steps 4-7 as TokenStore.rank_hits runs them (the read-back of the largest count included), host wall
  search_ms          the whole search_device call, host wall time with a device synchronise
  candidates_share   candidates_ms over the sum of the four stages
  host_glue_ms       steps 4-7 built only from what the library offered before this operator: the token hits copied to the
                     host, a Python set of documents per query (numpy searchsorted over the begin rows), TokenStore.aggregate
                     on the seq_id lists, a Python sort of its tuples; host wall time, same hits, same process
  candidates_mean    mean candidate documents per query
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops, synth  # noqa: E402
from matchmaker_amd.token_store import TokenStore  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=15_000,
                help="15,000 passages = 1.05 M token rows: ops.dot_topk draws a query's threshold from a 16,384-row sample at a "
                     "rank of at least 4, which it can place for k' = 128 up to about 1.3 M rows (2.5 k' 16384 / 4)")
ap.add_argument("--nq", type=int, nargs="+", default=[1, 64])
ap.add_argument("--token-top-k", type=int, nargs="+", default=[128, 512])
ap.add_argument("--top-n", type=int, default=1000)
ap.add_argument("--steps", type=int, default=5)
a = ap.parse_args()
Q, E, D = 32, 128, 180
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(3131)

lens = synth.msmarco_doc_lengths(a.docs, D, g, dev).long()
end = torch.cumsum(lens, 0)
begin = end - lens
T = int(end[-1])
tokens = torch.empty((T, E), dtype=torch.float16, device=dev)
for s0 in range(0, T, 1 << 24):
    n = min(1 << 24, T - s0)
    tokens[s0:s0 + n] = torch.nn.functional.normalize(torch.randn(n, E, generator=g, device=dev), dim=-1).half()
begin_h, end_h = begin.cpu().numpy(), end.cpu().numpy()
store = TokenStore(tokens, list(range(a.docs)), begin_h, end_h)


def wall_ms(fn, steps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_glue(q, hits, top_n):
    """dot_topk's rows -> .cpu() -> a Python set of documents per query -> aggregate -> sorted tuples."""
    rows = hits.cpu().numpy()
    cands = []
    for r in rows:
        r = r[r >= 0]
        j = np.searchsorted(begin_h, r, side="right") - 1
        cands.append(sorted(set(j[r < end_h[j]].tolist())))
    res = store.aggregate(q, cands, use_fp16=True)
    return [sorted(x, key=lambda t: (-t[1], t[0]))[:top_n] for x in res]


out = {"store": f"{a.docs} passages, {T} token rows, {T * E * 2 / 1e9:.2f} GB fp16, lengths N(70, 25) clipped to [8, {D}]",
       "Q": Q, "E": E, "top_n": a.top_n, "cases": []}
for nq in a.nq:
    q = torch.nn.functional.normalize(torch.randn(nq, Q, E, generator=g, device=dev), dim=-1).half()
    for k in a.token_top_k:
        hits = store.token_hits(q, k)
        cd, cb, ce, count = ops.colbert_candidates(hits, store._begin_sorted, store._end_sorted, store._doc_of_sorted, T)
        C = max(int(count.max()), 1)
        cd, cb, ce = cd[:, :C].contiguous(), cb[:, :C].contiguous(), ce[:, :C].contiguous()
        sc = ops.maxsim_ragged(q, tokens, cb.view(-1), ce.view(-1), None, pairs_per_query=C, check_ranges=False, sim_round=True)
        ids = cd.to(torch.int64)
        stage = {
            "token_search_ms": bench.gpu_time_ms(lambda: store.token_hits(q, k), a.steps),
            "candidates_ms": bench.gpu_time_ms(lambda: ops.colbert_candidates(hits, store._begin_sorted, store._end_sorted,
                                                                             store._doc_of_sorted, T), a.steps),
            "maxsim_ms": bench.gpu_time_ms(lambda: ops.maxsim_ragged(q, tokens, cb.view(-1), ce.view(-1), None, pairs_per_query=C,
                                                                     check_ranges=False, sim_round=True), a.steps),
            "selection_ms": bench.gpu_time_ms(lambda: ops.topk_merge(sc.view(nq, C).masked_fill(cd < 0, float("-inf")), ids,
                                                                     a.top_n), a.steps),
        }
        case = {"nq": nq, "token_top_k": k, "hits_per_query": Q * k, "candidates_mean": float(count.float().mean()),
                "candidate_slots": C, **stage}
        case["candidates_share"] = stage["candidates_ms"] / sum(stage.values())
        case["rank_hits_ms"] = wall_ms(lambda: store.rank_hits(q, hits, a.top_n), a.steps)
        case["search_ms"] = wall_ms(lambda: store.search_device(q, a.top_n, k), a.steps)
        case["host_glue_ms"] = wall_ms(lambda: host_glue(q, hits, a.top_n), max(1, min(a.steps, 3)))
        # the two paths rank the same documents
        s_dev, d_dev = store.rank_hits(q, hits, a.top_n)
        glue = host_glue(q, hits, a.top_n)
        case["same_ranking_as_host_glue"] = all([t[0] for t in glue[i]] == [j for j in d_dev[i].tolist() if j >= 0] for i in range(nq))
        out["cases"].append(case)
print(json.dumps(out))
