#!/usr/bin/env python
"""Benchmark of the IVF index (IVFFlatIPIndexer: probe selection by mm_dot_topk_fwd over the centroids + the list scan
mm_ivf_scan_fwd) against the flat index (FlatIPIndexer, mm_dot_topk_fwd) on the same tensors in the same process, on one
GPU.  Synthetic and self-contained: a mixture of Gaussians on the unit sphere (uniform noise has no IVF structure), by
default 1.1 M x 768 float16 (one rank's shard of the sharded 8.8 M collection) with nlist / nprobe in the ratio of the
reference's example (20000 / 500 = 2.5 % of the lists per query).  Prints ONE JSON line; per nq in {1, 256, 6980}:

  ivf_ms / flat_ms   search_device, median of per-call HIP events in steady state (bench.gpu_time_ms)
  scan_ms            the list scan alone on the same probes
  recall             mean overlap of the IVF ids with the flat ids at top_n
  scan_gflop, scan_gbytes, frac_mfma_peak, frac_hbm_peak
                     what the scan needs (2 E per scored (query, vector) pair; every probed list's bytes once + the queries
                     + the candidate scores written once and read back five times: four radix passes and the gather of
                     the selection) over the scan time, against bench.py's MFMA and HBM peaks; frac_calibrated_stream
                     is the same bytes against the box's own stream rate (ops.hbm_stream_probe over the vectors)
  launches           kernel launches + memsets of one scan (rounds x 6 + 3; the rounds are the host's worst case)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops  # noqa: E402
from matchmaker_amd.retrieval import FlatIPIndexer, IVFFlatIPIndexer  # noqa: E402

MFMA_PEAK_FLOPS, HBM_PEAK_GBPS = bench.MFMA_PEAK_16BIT, bench.HBM_PEAK_GBS

ap = argparse.ArgumentParser()
ap.add_argument("--vectors", type=int, default=1_100_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nlist", type=int, default=2500, help="the example's 20000 lists over 8.8 M vectors = 2500 per 1.1 M shard")
ap.add_argument("--nprobe", type=int, default=0, help="0 = 2.5 %% of nlist, the example's 500 / 20000")
ap.add_argument("--clusters", type=int, default=4000)
ap.add_argument("--top-n", type=int, default=1000)
ap.add_argument("--nq", type=int, nargs="+", default=[1, 256, 6980])
ap.add_argument("--train-fraction", type=float, default=0.25)
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


centres = torch.randn(a.clusters, a.dim, generator=g, device=dev)
centres /= centres.norm(dim=1, keepdim=True)
vec = sample(a.vectors)
ids = torch.arange(a.vectors, dtype=torch.int64, device=dev)
cfg = {"token_dim": a.dim, "faiss_ivf_list_count": a.nlist, "faiss_ivf_search_probe_count": nprobe}
flat = FlatIPIndexer(cfg, device=dev)
flat.index_resident(ids, vec)
ivf = IVFFlatIPIndexer(cfg, device=dev)
t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0[0].record()
ivf.train_resident(vec, a.train_fraction)
ivf.index_resident(ids, vec)
t0[1].record()
torch.cuda.synchronize()
lens = torch.diff(ivf.list_begin)
probe_ms = bench.gpu_time_ms(lambda: ops.hbm_stream_probe(ivf.vectors), a.steps)
stream_gbps = ivf.vectors.numel() * 2 // 8192 * 8192 / probe_ms / 1e6
res = {"bench": "ivf", "vectors": a.vectors, "dim": a.dim, "nlist": a.nlist, "nprobe": nprobe, "top_n": a.top_n,
       "build_s": round(t0[0].elapsed_time(t0[1]) / 1e3, 2), "list_len_max": int(lens.max()), "empty_lists": int((lens == 0).sum()),
       "calibrated_stream_GBps": round(stream_gbps, 1), "legs": []}
for nq in a.nq:
    q = sample(nq)
    s, i, probes = ivf.search_device(q, a.top_n, return_probes=True)
    fs, fi = flat.search_device(q, a.top_n)
    both = torch.cat([i, fi], 1).sort(dim=1).values
    recall = float((both[:, 1:] == both[:, :-1]).sum()) / (nq * a.top_n)
    cand = int(lens[probes.long()].sum())                                   # scored (query, vector) pairs
    probed = torch.zeros(a.nlist, dtype=torch.bool, device=dev)
    probed[probes.long().flatten()] = True
    nbytes = int(lens[probed].sum()) * a.dim * 2 + nq * a.dim * 2 + cand * 4 * 6
    ivf_ms = bench.gpu_time_ms(lambda: ivf.search_device(q, a.top_n), a.steps)
    scan_ms = bench.gpu_time_ms(lambda: ops.ivf_scan(q, ivf.vectors, ivf.list_begin, probes, a.top_n), a.steps)
    flat_ms = bench.gpu_time_ms(lambda: flat.search_device(q, a.top_n), a.steps)
    flop = 2.0 * a.dim * cand
    res["legs"].append({"nq": nq, "ivf_ms": round(ivf_ms, 3), "scan_ms": round(scan_ms, 3), "flat_ms": round(flat_ms, 3),
                        "flat_over_ivf": round(flat_ms / ivf_ms, 2), "recall": round(recall, 4),
                        "scored_fraction": round(cand / (nq * a.vectors), 4), "scan_gflop": round(flop / 1e9, 2),
                        "scan_gbytes": round(nbytes / 1e9, 3),
                        "frac_mfma_peak": round(flop / (scan_ms * 1e-3) / MFMA_PEAK_FLOPS, 4),
                        "frac_hbm_peak": round(nbytes / (scan_ms * 1e-3) / (HBM_PEAK_GBPS * 1e9), 4),
                        "frac_calibrated_stream": round(nbytes / (scan_ms * 1e-3) / (stream_gbps * 1e9), 4)})
print(json.dumps(res))
