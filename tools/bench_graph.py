#!/usr/bin/env python
"""Benchmark of the graph index (GraphIPIndexer: entry selection by mm_dot_topk_fwd over the entry sample + the beam search
mm_graph_search_fwd) against the flat index (FlatIPIndexer) and the IVF index (IVFFlatIPIndexer) on the same tensors in the
same process, on one GPU.  Same collection recipe as tools/bench_ivf.py: a mixture of Gaussians on the unit sphere, by default
1.1 M x 768 float16 (one rank's shard of the sharded 8.8 M collection).  Prints ONE JSON line.

  construction   per M: build_s = k-NN lists (ops.dot_topk of the shard against itself) + the graph (sorted torch ops)
  legs           per (M, top_n, nq), efSearch as given (ef = max(efSearch, top_n)):
    graph_ms / flat_ms / ivf_ms   search_device, median of per-call HIP events in steady state (bench.gpu_time_ms)
    entry_ms                      of graph_ms: the entry selection (top-k over the sample + the row mapping)
    iters, scored                 means of the kernel's stats (iterations run, rows scored)
    recall_at                     mean overlap of the graph's ids with the flat ids at 10 / 100 / top_n
    gather_GBps, frac_gather      rows scored x row bytes over the search kernel's time, and that rate as a fraction of
                                  5.5 TB/s: the rate at which random whole rows are gathered into registers from a buffer
                                  far larger than the Infinity Cache (four rows in flight per wavefront, 16 wavefronts per
                                  CU).  That figure was measured with rows of 1,152 B (5.7-5.8 TB/s with 2,304 B); the
                                  default rows here are 1,536 B, between the two: the fraction is against a figure taken
                                  at another row size
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops  # noqa: E402
from matchmaker_amd.retrieval import FlatIPIndexer, GraphIPIndexer, IVFFlatIPIndexer  # noqa: E402

GATHER_GBPS = 5500.0

ap = argparse.ArgumentParser()
ap.add_argument("--vectors", type=int, default=1_100_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--clusters", type=int, default=4000)
ap.add_argument("--neighbors", type=int, nargs="+", default=[32, 128])
ap.add_argument("--ef-search", type=int, default=128)
ap.add_argument("--top-n", type=int, nargs="+", default=[100, 1000])
ap.add_argument("--nq", type=int, nargs="+", default=[1, 16, 256, 6980])
ap.add_argument("--nlist", type=int, default=2500)
ap.add_argument("--nprobe", type=int, default=0, help="0 = 2.5 %% of nlist")
ap.add_argument("--train-fraction", type=float, default=0.25)
ap.add_argument("--no-ivf", action="store_true")
ap.add_argument("--steps", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
nprobe = a.nprobe or max(1, round(a.nlist * 0.025))
g = torch.Generator(device=dev).manual_seed(0)


def sample(n):
    """centre + noise of the centre's own length, back on the sphere"""
    out = torch.empty((n, a.dim), dtype=torch.float16, device=dev)
    for lo in range(0, n, 1 << 17):
        m = min(1 << 17, n - lo)
        x = centres[torch.randint(0, a.clusters, (m,), generator=g, device=dev)]
        x = x + torch.randn(m, a.dim, generator=g, device=dev) / a.dim ** 0.5
        out[lo: lo + m] = (x / x.norm(dim=1, keepdim=True)).half()
    return out


def timed(fn):
    t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t[0].record()
    r = fn()
    t[1].record()
    torch.cuda.synchronize()
    return r, t[0].elapsed_time(t[1]) / 1e3


def overlap(x, y, k):
    both = torch.cat([x[:, :k], y[:, :k]], 1).sort(dim=1).values
    return float(((both[:, 1:] == both[:, :-1]) & (both[:, 1:] >= 0)).sum()) / (x.shape[0] * k)


centres = torch.randn(a.clusters, a.dim, generator=g, device=dev)
centres /= centres.norm(dim=1, keepdim=True)
vec = sample(a.vectors)
ids = torch.arange(a.vectors, dtype=torch.int64, device=dev)
queries = {nq: sample(nq) for nq in a.nq}
cfg = {"token_dim": a.dim, "faiss_ivf_list_count": a.nlist, "faiss_ivf_search_probe_count": nprobe}
flat = FlatIPIndexer(cfg, device=dev)
flat.index_resident(ids, vec)
res = {"bench": "graph", "vectors": a.vectors, "dim": a.dim, "ef_search": a.ef_search, "nlist": a.nlist, "nprobe": nprobe,
       "gather_GBps_guide": GATHER_GBPS, "construction": [], "legs": []}
ivf = None
if not a.no_ivf:
    ivf = IVFFlatIPIndexer(cfg, device=dev)
    _, res["ivf_build_s"] = timed(lambda: (ivf.train_resident(vec, a.train_fraction), ivf.index_resident(ids, vec)))
    res["ivf_build_s"] = round(res["ivf_build_s"], 2)
base = {}
for top_n in a.top_n:
    for nq in a.nq:
        q = queries[nq]
        fi = flat.search_device(q, top_n)[1]
        base[(top_n, nq)] = (fi, bench.gpu_time_ms(lambda: flat.search_device(q, top_n), a.steps),
                             bench.gpu_time_ms(lambda: ivf.search_device(q, top_n), a.steps) if ivf is not None else None)
for M in a.neighbors:
    ix = GraphIPIndexer({"token_dim": a.dim, "faiss_hnsw_graph_neighbors": M, "faiss_hnsw_efSearch": a.ef_search,
                         "faiss_hnsw_efConstruction": 128}, device=dev)
    _, build_s = timed(lambda: ix.index_resident(ids, vec))
    deg = (ix.neighbors >= 0).sum(1).float()
    res["construction"].append({"M": M, "build_s": round(build_s, 2), "mean_degree": round(float(deg.mean()), 2)})
    print(json.dumps(res["construction"][-1]), file=sys.stderr, flush=True)
    for top_n in a.top_n:
        ef = max(a.ef_search, top_n)
        for nq in a.nq:
            q = queries[nq]
            fi, flat_ms, ivf_ms = base[(top_n, nq)]
            entry = ix.entry_rows(q, ef)
            s, rows, st = ops.graph_search(q, ix.vectors, ix.neighbors, entry, ef, top_n, ix.width, return_stats=True)
            gi = ix.search_device(q, top_n)[1]
            graph_ms = bench.gpu_time_ms(lambda: ix.search_device(q, top_n), a.steps)
            entry_ms = bench.gpu_time_ms(lambda: ix.entry_rows(q, ef), a.steps)
            kern_ms = bench.gpu_time_ms(lambda: ops.graph_search(q, ix.vectors, ix.neighbors, entry, ef, top_n, ix.width), a.steps)
            scored = float(st[:, 1].float().mean())
            rate = scored * nq * a.dim * 2 / (kern_ms * 1e-3) / 1e9
            leg = {"M": M, "top_n": top_n, "nq": nq, "ef": ef, "graph_ms": round(graph_ms, 3), "entry_ms": round(entry_ms, 3),
                   "kernel_ms": round(kern_ms, 3), "flat_ms": round(flat_ms, 3), "iters": round(float(st[:, 0].float().mean()), 1),
                   "scored": round(scored, 1),
                   "recall_at": {str(k): round(overlap(gi, fi, k), 4) for k in sorted({10, min(100, top_n), top_n})},
                   "gather_GBps": round(rate, 1), "frac_gather": round(rate / GATHER_GBPS, 4),
                   "flat_over_graph": round(flat_ms / graph_ms, 2)}
            if ivf_ms is not None:
                leg["ivf_ms"] = round(ivf_ms, 3)
                leg["ivf_over_graph"] = round(ivf_ms / graph_ms, 2)
            res["legs"].append(leg)
            print(json.dumps(leg), file=sys.stderr, flush=True)       # progress; the record is the last stdout line
    del ix
    torch.cuda.empty_cache()
print(json.dumps(res))
