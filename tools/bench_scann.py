#!/usr/bin/env python
"""Benchmark of the quantized index (ScannIPIndexer: probe selection by mm_dot_topk_fwd over the leaf centres, the scan of
the 4-bit codes mm_ah_scan_fwd, the exact re-score mm_gather_dot, mm_topk_merge) on one GPU, with the flat index
(FlatIPIndexer) as the truth for recall and the IVF list scan (mm_ivf_scan_fwd) of the SAME probes over the SAME
list-ordered float16 rows as the yardstick.  Synthetic and self-contained: tools/bench_ivf.py's collection, a mixture of
Gaussians on the unit sphere, by default 1.1 M x 768 float16 (one rank's shard of the sharded 8.8 M collection), with the
reference's constants: int(sqrt(n)) leaves, 100 searched, reorder = top_n.  Prints ONE JSON line; per (nq, top_n):

  search_ms                   search_device, median of per-call HIP events in steady state (bench.gpu_time_ms)
  probe_ms, scan_ms, rescore_ms, merge_ms
                              the four stages alone on the same tensors
  score_ms, select_ms         the scan split by kernel (ah_score_kernel / ivf_select_kernel): device time per call from
                              torch.profiler in a pass of its own, null when the profiler reports no such kernel
  ivf_scan_ms, ivf_score_ms, ivf_select_ms, scan_over_ivf
                              mm_ivf_scan_fwd with k = top_n on the same probes; scan_over_ivf > 1 = the code scan is SLOWER
  recall_scan, recall         mean overlap with the flat ids at top_n: of the top_n rows by quantized score, and of the
                              result after the re-score
  score_gbytes, score_gflop, frac_hbm_peak, frac_mfma_peak
                              what the score stage needs — every probed leaf's codes once, the codebook once per
                              workgroup, the queries once, the candidate scores written once; 2 E per scored (query, row)
                              pair — over score_ms (over scan_ms, and named so in `fraction_of`, when the split is missing)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops  # noqa: E402
from matchmaker_amd.retrieval import FlatIPIndexer, ScannIPIndexer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--vectors", type=int, default=1_100_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--clusters", type=int, default=4000)
ap.add_argument("--top-n", type=int, nargs="+", default=[100, 1000])
ap.add_argument("--nq", type=int, nargs="+", default=[1, 256, 6980])
ap.add_argument("--steps", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
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


def kernel_ms(fn, names):
    """device milliseconds per call of the kernels whose name holds one of `names`, from one profiled call"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for n in names:
            us = [e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
                  for e in prof.key_averages() if n in e.key]
            out[n] = round(sum(us) / 1e3, 3) if us else None
        return out
    except Exception as e:      # no profiler: the split is not measured
        return {n: None for n in names} | {"error": repr(e)}


def overlap(i, fi):
    both = torch.cat([i, fi], 1).sort(dim=1).values
    return float(((both[:, 1:] == both[:, :-1]) & (both[:, 1:] >= 0)).sum()) / fi.numel()


centres = torch.randn(a.clusters, a.dim, generator=g, device=dev)
centres /= centres.norm(dim=1, keepdim=True)
vec = sample(a.vectors)
ids = torch.arange(a.vectors, dtype=torch.int64, device=dev)
cfg = {"token_dim": a.dim, "token_dtype": "float16", "query_sets": {"bench": {"top_n": max(a.top_n)}}}
flat = FlatIPIndexer(cfg, device=dev)
flat.index_resident(ids, vec)
ix = ScannIPIndexer(cfg, device=dev)
t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0[0].record()
ix.index_resident(ids, vec)
t0[1].record()
torch.cuda.synchronize()
t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t1[0].record()
ops.ah_encode(ix.vectors, torch.repeat_interleave(torch.arange(ix.nlist, device=dev, dtype=torch.int32), torch.diff(ix.list_begin)),
              ix.centroids, ix.codebook, ix.eta, ix.DESCENT_PASSES)
t1[1].record()
torch.cuda.synchronize()
lens = torch.diff(ix.list_begin)
nprobe = min(ix.leaves_to_search, ix.nlist)
res = {"bench": "scann", "vectors": a.vectors, "dim": a.dim, "leaves": ix.nlist, "leaves_searched": nprobe, "eta": round(ix.eta, 3),
       "build_s": round(t0[0].elapsed_time(t0[1]) / 1e3, 2), "encode_s": round(t1[0].elapsed_time(t1[1]) / 1e3, 3),
       "leaf_len_max": int(lens.max()), "empty_leaves": int((lens == 0).sum()),
       "code_bytes_per_row": a.dim // 4, "row_bytes": a.dim * 2, "legs": []}
for nq in a.nq:
    q = sample(nq)
    for top_n in a.top_n:
        ix.reorder = top_n
        s, i, (probes, qs, rows, exact) = ix.search_device(q, top_n, return_stages=True)
        ps = ops.dot_topk(q, ix.centroids, nprobe)[0]
        fs, fi = flat.search_device(q, top_n)
        scan_ids = torch.where(rows[:, :top_n] >= 0, ix.ids[rows[:, :top_n].clamp(min=0)], rows[:, :top_n])
        cand = int(lens[probes.long()].sum())                                   # scored (query, row) pairs
        probed = torch.zeros(ix.nlist, dtype=torch.bool, device=dev)
        probed[probes.long().flatten()] = True
        tasks = int(((lens + 31) // 32).sum())
        wgs = min((tasks + 3) // 4, 1024)
        nbytes = int(lens[probed].sum()) * (a.dim // 4) + wgs * 32 * a.dim + nq * a.dim * 2 + cand * 4
        flop = 2.0 * a.dim * cand

        def scan():
            return ops.ah_scan(q, ix.codes, ix.codebook, ix.list_begin, probes, ps, top_n)

        def ivf():
            return ops.ivf_scan(q, ix.vectors, ix.list_begin, probes, top_n)

        search_ms = bench.gpu_time_ms(lambda: ix.search_device(q, top_n), a.steps)
        probe_ms = bench.gpu_time_ms(lambda: ops.dot_topk(q, ix.centroids, nprobe), a.steps)
        scan_ms = bench.gpu_time_ms(scan, a.steps)
        rescore_ms = bench.gpu_time_ms(lambda: ops.gather_dot(q, ix.vectors, rows), a.steps)
        merge_ms = bench.gpu_time_ms(lambda: ops.topk_merge(exact, rows, top_n), a.steps)
        ivf_ms = bench.gpu_time_ms(ivf, a.steps)
        ks = kernel_ms(scan, ["ah_score_kernel", "ivf_select_kernel"])
        ki = kernel_ms(ivf, ["ivf_score_kernel", "ivf_select_kernel"])
        over = ks["ah_score_kernel"] or scan_ms
        res["legs"].append({
            "nq": nq, "top_n": top_n, "search_ms": round(search_ms, 3), "probe_ms": round(probe_ms, 3), "scan_ms": round(scan_ms, 3),
            "score_ms": ks["ah_score_kernel"], "select_ms": ks["ivf_select_kernel"], "rescore_ms": round(rescore_ms, 3),
            "merge_ms": round(merge_ms, 3), "ivf_scan_ms": round(ivf_ms, 3), "ivf_score_ms": ki["ivf_score_kernel"],
            "ivf_select_ms": ki["ivf_select_kernel"], "scan_over_ivf": round(scan_ms / ivf_ms, 2),
            "recall_scan": round(overlap(scan_ids, fi), 4), "recall": round(overlap(i, fi), 4),
            "scored_fraction": round(cand / (nq * a.vectors), 4), "score_gbytes": round(nbytes / 1e9, 3),
            "score_gflop": round(flop / 1e9, 2), "fraction_of": "score_ms" if ks["ah_score_kernel"] else "scan_ms",
            "frac_hbm_peak": round(nbytes / (over * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), 4),
            "frac_mfma_peak": round(flop / (over * 1e-3) / bench.MFMA_PEAK_16BIT, 4),
            **({"profiler_error": ks["error"]} if "error" in ks else {})})
print(json.dumps(res))
