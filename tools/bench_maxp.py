#!/usr/bin/env python
"""Benchmark of MaxP retrieval's aggregation (ops.distinct_hits = mm_distinct_hits_fwd, retrieval.MaxPIndexer) on
one GPU, in one process, on synthetic hits only.  Prints ONE JSON line:

  legs[]     nq 1 / 64 / 6,980 x K 1,000 / 8,192 hits, top_n 100 / 1,000; a query's hits are passages of a window of a
             collection whose documents have 1-40 passages, so a list holds a few hundred to a few thousand documents:
               kernel_ms         ops.distinct_hits alone, HIP events in steady state (bench.gpu_time_ms)
               torch_ms          the device-only torch formulation on the same hits: stable sort by id, neighbour compare,
                                 scatter to positions, cumsum, scatter of the kept hits (torch_distinct below)
               host_loop_ms      the reference's loop (dense_retrieval.py:414-429: set, first hit per id, break at top_n) on
                                 the hits copied to the host, the copy included; timed on at most 256 queries and scaled to
                                 nq (host_loop_queries_timed says how many ran)
               frac_hbm_peak     (nq K 12 read + the outputs written) bytes over kernel_ms against the nominal HBM peak
               same_as_torch     the two device results are bit-equal
  indexer    MaxPIndexer.search_device (top_n 100 of K 1,000 hits) over a resident FlatIPIndexer of ~1.1 M x 768 fp16
             passages against inner.search_device(K) alone, host clock around synchronised calls: the share the dedupe adds
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


def torch_distinct(s, ids, top_n):
    """ops.distinct_hits' (scores, ids, pos, n_distinct, n_valid) from torch operators alone."""
    nq, K = ids.shape
    sorted_ids, order = torch.sort(ids, dim=1, stable=True)                  # negative ids first; equal ids in list order
    first = torch.ones_like(sorted_ids, dtype=torch.bool)
    first[:, 1:] = sorted_ids[:, 1:] != sorted_ids[:, :-1]
    first &= sorted_ids >= 0
    flag = torch.zeros_like(first).scatter_(1, order, first)                 # by position
    rank = torch.cumsum(flag, 1) - 1
    slot = torch.where(flag & (rank < top_n), rank, torch.full_like(rank, top_n))      # slot top_n: thrown away
    pos = torch.arange(K, device=ids.device, dtype=torch.int32).expand(nq, K)
    out_s = torch.full((nq, top_n + 1), float("-inf"), dtype=s.dtype, device=s.device).scatter_(1, slot, s)[:, :top_n]
    out_i = torch.full((nq, top_n + 1), -1, dtype=ids.dtype, device=s.device).scatter_(1, slot, ids)[:, :top_n]
    out_p = torch.full((nq, top_n + 1), -1, dtype=torch.int32, device=s.device).scatter_(1, slot, pos)[:, :top_n]
    return out_s, out_i, out_p, flag.sum(1).to(torch.int32), (ids >= 0).sum(1).to(torch.int32)


def host_loop(scores, ids, top_n):
    """dense_retrieval.py:414-429 on host arrays: [[(id, score), ...] per query]."""
    results = []
    for q in range(ids.shape[0]):
        current_scores, current_ids = scores[q], ids[q]
        unique_ids, found = set(), []
        for t, s_idx in enumerate(current_ids):
            if s_idx in unique_ids:
                continue
            unique_ids.add(s_idx)
            found.append((s_idx, float(current_scores[t])))
            if len(found) == top_n:
                break
        results.append(found)
    return results


def host_ms(fn, reps):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        best = ms if best is None else min(best, ms)
    return best


def make_hits(doc_of, nq, K, gen, dev):
    """Every query's hits: K passages drawn from a window of 4 K consecutive passages of the collection, scores descending."""
    P = doc_of.shape[0]
    start = torch.randint(0, P - 4 * K, (nq, 1), generator=gen, device=dev)
    rows = start + torch.randint(0, 4 * K, (nq, K), generator=gen, device=dev)
    s = torch.sort(torch.randn((nq, K), generator=gen, device=dev), dim=1, descending=True).values
    return s.contiguous(), doc_of[rows].contiguous()


def main():
    from matchmaker_amd import ops
    from matchmaker_amd.retrieval import FlatIPIndexer, MaxPIndexer
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--passages", type=int, default=1_100_000)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(414)
    P = 60_000 if a.small else a.passages
    sizes = torch.randint(1, 41, (P // 20,), generator=gen, device=dev)         # 1-40 passages per document
    doc_of = torch.repeat_interleave(torch.arange(sizes.numel(), device=dev), sizes)
    P = doc_of.shape[0]
    shapes = [(2, 100, 10)] if a.small else [(nq, K, top_n) for nq in (1, 64, 6980) for K in (1000, 8192) for top_n in (100, 1000)]
    out = {"passages": P, "documents": int(sizes.numel()), "hbm_peak_GBps": bench.HBM_PEAK_GBS, "legs": []}
    for nq, K, top_n in shapes:
        s, ids = make_hits(doc_of, nq, K, gen, dev)
        got, ref = ops.distinct_hits(s, ids, top_n), torch_distinct(s, ids, top_n)
        same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(got, ref))
        k_ms, t_ms = [], []
        for _ in range(2):                                                      # alternated; the first round also warms
            k_ms.append(bench.gpu_time_ms(lambda: ops.distinct_hits(s, ids, top_n), a.steps))
            t_ms.append(bench.gpu_time_ms(lambda: torch_distinct(s, ids, top_n), a.steps))
        nh = min(nq, 256)
        h_ms = host_ms(lambda: host_loop(s[:nh].cpu().numpy(), ids[:nh].cpu().numpy(), top_n), 1) * nq / nh
        nbytes = nq * K * 12 + nq * top_n * 16 + nq * 8
        out["legs"].append({"queries": nq, "hits": K, "top_n": top_n, "kernel_ms": min(k_ms), "torch_ms": min(t_ms),
                            "torch_over_kernel": min(t_ms) / min(k_ms), "both_rounds_ms": {"kernel": k_ms, "torch": t_ms},
                            "host_loop_ms": h_ms, "host_loop_queries_timed": nh, "host_loop_over_kernel": h_ms / min(k_ms),
                            "mean_distinct": float(got[3].float().mean()), "bytes": nbytes,
                            "frac_hbm_peak": nbytes / (min(k_ms) * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), "same_as_torch": bool(same)})
        del s, ids, got, ref
        torch.cuda.empty_cache()
    # the indexer: what the dedupe adds to a search
    E, nq, K, top_n = (128, 8, 100, 10) if a.small else (768, 64, 1000, 100)
    vec = torch.empty((P, E), dtype=torch.float16, device=dev)
    for lo in range(0, P, 1 << 17):
        vec[lo: lo + (1 << 17)] = torch.randn((min(1 << 17, P - lo), E), generator=gen, device=dev).to(torch.float16)
    ix = MaxPIndexer(FlatIPIndexer({"token_dim": E}, device=dev), max_hits=4096)
    ix.index_resident(doc_of, vec)
    q = torch.randn((nq, E), generator=gen, device=dev).to(torch.float16)
    inner, both = [], []
    for _ in range(3):                                                          # alternated; the first round warms
        inner.append(host_ms(lambda: ix.inner.search_device(q, K), 2))
        both.append(host_ms(lambda: ix.search_device(q, top_n, index_hit_top_n=K), 2))
    _, _, info = ix.search_device(q, top_n, index_hit_top_n=K, return_info=True)
    out["indexer"] = {"passages": P, "dim": E, "queries": nq, "hits": K, "top_n": top_n, "inner_search_ms": min(inner[1:]),
                      "maxp_search_ms": min(both[1:]), "dedupe_share": 1.0 - min(inner[1:]) / min(both[1:]),
                      "all_rounds_ms": {"inner": inner, "maxp": both}, "complete": int(info["complete"].sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
