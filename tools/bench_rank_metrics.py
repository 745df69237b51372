#!/usr/bin/env python
"""Benchmark of the device-side ranking and IR metrics (matchmaker_amd.metrics.EvalSet over ops.segment_rank / rank_metrics /
rank_metrics_depth) on one GPU, in one process, on synthetic data only (integer ids, three judged documents
per query, first-stage ranks a random permutation).  Prints ONE JSON line:

  plain[]   ranking + calculate_metrics_plain at 256 x 1000 and 6,980 x 1000 (queries x candidates):
              rank_ms / metrics_ms      ops.segment_rank / ops.rank_metrics alone, HIP events in steady state (bench.gpu_time_ms)
              torch_sort_ms             yardstick for the ranking alone: torch.sort(stable=True, descending=True) over the
                                        padded [nq, max_len] score matrix on the device
              native_end_to_end_ms      EvalSet.metrics_plain(scores): both kernels, the read-back of the per-query arrays and
                                        the dict (host clock around a synchronised call)
              numpy_end_to_end_ms       the module's numpy route on the same device scores (native=False): the path replaced
  depth[]   calculate_metrics_along_candidate_depth at 64 x 1000 over [1, 1000] and 6,980 x 100 over [1, 100]:
              sweep_ms                  ops.rank_metrics_depth alone (one launch, all queries)
              native_end_to_end_ms / numpy_end_to_end_ms   EvalSet.metrics_along_candidate_depth, both routes
  same_as_numpy  the native dicts against the numpy route's (means within 1e-12 relative, everything else equal)
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
from matchmaker_amd import ops  # noqa: E402
from matchmaker_amd.metrics import EvalSet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=2)
ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
a = ap.parse_args()
dev = torch.device("cuda:0")
PLAIN = [(8, 50)] if a.small else [(256, 1000), (6980, 1000)]
DEPTH = [(4, 50)] if a.small else [(64, 1000), (6980, 100)]


def make_set(nq, depth, seed):
    rng = np.random.default_rng(seed)
    qids = np.repeat(np.arange(nq), depth).tolist()
    dids = np.tile(np.arange(depth), nq).tolist()
    qrels = {q: {int(d): int(g) for d, g in zip(rng.permutation(depth)[:3], (1, 1, 2))} for q in range(nq)}
    cand = {q: dict(zip(range(depth), (rng.permutation(depth) + 1).tolist())) for q in range(nq)}
    t0 = time.perf_counter()
    es = EvalSet(qids, dids, qrels, cand)
    return es.to(dev), 1e3 * (time.perf_counter() - t0)


def host_ms(fn, reps):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        best = ms if best is None else min(best, ms)
    return best, out


def same(x, y):
    if isinstance(next(iter(x.values())), dict):
        return list(x) == list(y) and all(same(x[k], y[k]) for k in x)
    ok = list(x) == list(y)
    for k in x:
        u, v = float(x[k]), float(y[k])
        ok = ok and ((np.isnan(u) and np.isnan(v)) or abs(u - v) <= 1e-12 * abs(v))
    return bool(ok)


def plain_leg(nq, depth):
    es, build_ms = make_set(nq, depth, 5)
    g = torch.Generator(device=dev).manual_seed(11)
    scores = torch.randn(nq * depth, generator=g, device=dev)
    t = es.t
    order = ops.segment_rank(scores, t["seg_begin"], es.max_len)
    margs = (order, t["seg_begin"], t["grade"], None, 2 ** 31 - 1, 1.0, es.rcut, es.ncut, es.map_cut, t["bnr"], t["idcg"], t["log2"])
    padded = scores.view(nq, depth)
    r, m, s = [], [], []
    for _ in range(2):                                                     # alternated; the first round also warms
        s.append(bench.gpu_time_ms(lambda: torch.sort(padded, dim=1, descending=True, stable=True), a.steps))
        r.append(bench.gpu_time_ms(lambda: ops.segment_rank(scores, t["seg_begin"], es.max_len), a.steps))
        m.append(bench.gpu_time_ms(lambda: ops.rank_metrics(*margs), a.steps))
    tidx = torch.sort(padded, dim=1, descending=True, stable=True)[1] + torch.arange(nq, device=dev)[:, None] * depth
    nat, d_nat = host_ms(lambda: es.metrics_plain(scores), a.host_reps)
    npy, d_np = host_ms(lambda: es.metrics_plain(scores, native=False), a.host_reps)
    return {"queries": nq, "candidates": depth, "evalset_build_ms": build_ms, "rank_ms": min(r), "metrics_ms": min(m),
            "torch_sort_ms": min(s), "rank_over_torch_sort": min(r) / min(s), "both_rounds_ms": {"rank": r, "metrics": m, "torch_sort": s},
            "order_equals_torch_sort": bool(torch.equal(order.view(nq, depth).long(), tidx)),
            "native_end_to_end_ms": nat, "numpy_end_to_end_ms": npy, "numpy_over_native": npy / nat, "same_as_numpy": same(d_nat, d_np)}


def depth_leg(nq, depth):
    es, build_ms = make_set(nq, depth, 6)
    g = torch.Generator(device=dev).manual_seed(12)
    scores = torch.randn(nq * depth, generator=g, device=dev)
    t = es.t
    order = ops.segment_rank(scores, t["seg_begin"], es.max_len)
    dargs = (order, t["seg_begin"], t["grade"], t["cand_pos"], depth, 1.0, es.rcut, es.ncut, es.map_cut, t["bnr"], t["idcg"], t["log2"])
    sw = [bench.gpu_time_ms(lambda: ops.rank_metrics_depth(*dargs), a.steps) for _ in range(2)]
    nat, d_nat = host_ms(lambda: es.metrics_along_candidate_depth(scores, (1, depth)), a.host_reps)
    npy, d_np = host_ms(lambda: es.metrics_along_candidate_depth(scores, (1, depth), native=False), max(1, a.host_reps - 1))
    return {"queries": nq, "candidates": depth, "range": [1, depth], "evalset_build_ms": build_ms, "sweep_ms": min(sw),
            "both_rounds_ms": sw, "output_bytes": nq * depth * (4 + 4 * len(es.rcut) + 8 + 8 * len(es.ncut)),
            "native_end_to_end_ms": nat, "numpy_end_to_end_ms": npy, "numpy_over_native": npy / nat, "same_as_numpy": same(d_nat, d_np)}


out = {"plain": [], "depth": []}
for nq, depth in PLAIN:
    out["plain"].append(plain_leg(nq, depth))
    torch.cuda.empty_cache()
for nq, depth in DEPTH:
    out["depth"].append(depth_leg(nq, depth))
    torch.cuda.empty_cache()
print(json.dumps(out))
