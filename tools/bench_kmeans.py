#!/usr/bin/env python
"""Benchmark of the native k-means path (ops.kmeans_assign = mm_kmeans_assign, ops.kmeans_segment_sum =
mm_kmeans_segment_sum, retrieval.spherical_kmeans) against the present one (IVFFlatIPIndexer._train with
native_kmeans=False: ops.dot_topk(k = 1) per 16,384 vectors + index_add_ over fp32 copies) on the same tensors, on the same
GPU and in the same process.  Synthetic and self-contained: a mixture of Gaussians on the unit sphere.

Without --shape every shape runs as a child process of its own under `timeout` (a shape that fails or hangs ends the run:
nothing else is started on the GPU after it); with --shape NAME the shape is measured here.  One JSON line per shape:

  present_assign_ms / native_assign_ms   one assignment of all vectors, median of per-call HIP events (bench.gpu_time_ms)
  present_sums_ms / native_sums_ms       the centroid update: per-list sums + counts + normalisation (native: including the
                                         stable sort of the assignment that yields order / list_begin)
  segment_sum_ms                         ops.kmeans_segment_sum alone
  present_iter_ms / native_iter_ms       assignment + update
  present_prepare_s / native_prepare_s   train_resident on all vectors: KMEANS_ITERS iterations, host clock around a synchronise
  assign_frac_mfma_peak                  2 n nlist E flop over native_assign_ms against the nominal 16-bit MFMA peak
  sums_frac_hbm_peak                     (2 n E + 4 nlist E) bytes over segment_sum_ms against the nominal HBM peak
  assign_agreement                       fraction of vectors both paths put into the same list (they differ on near-ties only)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {                       # name -> (vectors, dim, lists, seconds allowed)
    "clusterer": (400_000, 768, 2000, 300),        # query_clusterer.py: the query set of TAS-Balanced
    "ivf_shard": (1_100_000, 768, 2500, 420),      # tools/bench_ivf.py's shard
    "token_store": (1_050_000, 128, 4096, 300),    # the token store of tools/bench_colbert_search.py
}


def measure(name, steps):
    import torch
    import bench
    from matchmaker_amd import ops
    from matchmaker_amd.retrieval import IVFFlatIPIndexer, _lists_of, _unit_rows

    n, E, nlist, _ = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn(nlist, E, generator=g, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    x = torch.empty((n, E), dtype=torch.float16, device=dev)
    for lo in range(0, n, 1 << 17):
        m = min(1 << 17, n - lo)
        v = centres[torch.randint(0, nlist, (m,), generator=g, device=dev)] + torch.randn(m, E, generator=g, device=dev) / E ** 0.5
        x[lo: lo + m] = (v / v.norm(dim=1, keepdim=True)).half()
    cfg = {"token_dim": E, "faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": 1}
    old = IVFFlatIPIndexer(cfg, device=dev)
    new = IVFFlatIPIndexer(cfg, device=dev, native_kmeans=True)
    cent = _unit_rows(x[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:nlist].to(dev)].float()).half()

    a_old = old._assign(x, cent)
    a_new = ops.kmeans_assign(x, cent)[0].to(torch.int64)

    def present_sums():
        sums = torch.zeros((nlist, E), dtype=torch.float32, device=dev)
        for lo in range(0, n, old.SUM_CHUNK):
            sums.index_add_(0, a_old[lo: lo + old.SUM_CHUNK], x[lo: lo + old.SUM_CHUNK].float())
        torch.bincount(a_old, minlength=nlist)
        return _unit_rows(sums).half()

    def native_sums():
        order, lb, _ = _lists_of(a_new, nlist)
        return _unit_rows(ops.kmeans_segment_sum(x, order, lb)).half()

    order, lb, _ = _lists_of(a_new, nlist)
    t = {"present_assign_ms": bench.gpu_time_ms(lambda: old._assign(x, cent), steps),
         "native_assign_ms": bench.gpu_time_ms(lambda: ops.kmeans_assign(x, cent), steps),
         "present_sums_ms": bench.gpu_time_ms(present_sums, steps),
         "native_sums_ms": bench.gpu_time_ms(native_sums, steps),
         "segment_sum_ms": bench.gpu_time_ms(lambda: ops.kmeans_segment_sum(x, order, lb), steps)}

    def prepare_s(ix):
        ix.train_resident(x)                                     # warm: allocator, code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.train_resident(x)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {"bench": "kmeans", "shape": name, "vectors": n, "dim": E, "nlist": nlist, "iters": old.KMEANS_ITERS}
    res.update({k: round(v, 3) for k, v in t.items()})
    res["present_iter_ms"] = round(t["present_assign_ms"] + t["present_sums_ms"], 3)
    res["native_iter_ms"] = round(t["native_assign_ms"] + t["native_sums_ms"], 3)
    res["iter_speedup"] = round(res["present_iter_ms"] / res["native_iter_ms"], 2)
    res["present_prepare_s"] = round(prepare_s(old), 3)
    res["native_prepare_s"] = round(prepare_s(new), 3)
    res["prepare_speedup"] = round(res["present_prepare_s"] / res["native_prepare_s"], 2)
    res["assign_frac_mfma_peak"] = round(2.0 * n * nlist * E / (t["native_assign_ms"] * 1e-3) / bench.MFMA_PEAK_16BIT, 4)
    res["sums_frac_hbm_peak"] = round((2.0 * n * E + 4.0 * nlist * E) / (t["segment_sum_ms"] * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), 4)
    res["assign_agreement"] = round(float((a_old == a_new).float().mean()), 6)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), help="measure this shape in this process")
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    if a.shape:
        measure(a.shape, a.steps)
        sys.exit(0)
    for name in a.shapes:
        cmd = ["timeout", "-k", "10", str(SHAPES[name][3]), sys.executable, os.path.abspath(__file__), "--shape", name,
               "--steps", str(a.steps)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(json.dumps({"bench": "kmeans", "shape": name, "error": f"exit status {rc}: not measured; stopping"}), flush=True)
            sys.exit(rc)
