#!/usr/bin/env python
"""Benchmark of the fp8 IVF list scan (ops.ivf_scan_fp8) and of the token index TokenStore.build_token_index gives an
fp8-only store (retrieval.IVFFp8IPIndexer), on one GPU, in one process.  The stores are tools/bench_fp8_token_search.py's
(DESIGN §3.18): store 1 = --docs MSMARCO-length passages at dim 128, store 2 = --docs768 at dim 768, unit fp16 token vectors,
quantised.  HIP events in steady state (bench.gpu_time_ms), the kernels of a comparison alternated.  Prints ONE JSON line:

  scan[]        per store (nlist 4096 / 1024), nprobe (16, 64), query-token count (32, 2048) and k' (128, 512):
                fp8_ms = ops.ivf_scan_fp8 over the index's lists, fp16_ms = ops.ivf_scan over ops.fp8_dequantize_rows of them
                with the SAME lists and probes (the yardstick: equal values, equal work), their ratio whatever it is, whether
                the two results agree (rows per query as sets), flat_fp8_ms = ops.dot_topk_fp8 over the whole store, and the
                mean overlap of the scan's hits with the flat fp8 hits (the recall of probing nprobe lists)
  end_to_end    search_device for 1 and 64 queries of 32 tokens on the fp8-ONLY store of store 1: index= against
                token_search="fp8"
  resident      bytes of store + token index for the three forms of DESIGN §3.19's table, at this tool's scale
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops, synth  # noqa: E402
from matchmaker_amd.token_store import TokenStore  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=15_000)
ap.add_argument("--docs768", type=int, default=2_500)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--subsample", type=float, default=-1, help="fraction of the rows the centroids are trained on")
a = ap.parse_args()
Q, D = 32, 180
dev = torch.device("cuda:0")


def unit_rows(n, E, g):
    out = torch.empty((n, E), dtype=torch.float16, device=dev)
    step = (1 << 28) // E
    for s0 in range(0, n, step):
        m = min(step, n - s0)
        out[s0:s0 + m] = torch.nn.functional.normalize(torch.randn(m, E, generator=g, device=dev), dim=-1).half()
    return out


def make_store(n_docs, E, g):
    lens = synth.msmarco_doc_lengths(n_docs, D, g, dev).long()
    end = torch.cumsum(lens, 0)
    begin = end - lens
    return unit_rows(int(end[-1]), E, g), begin, end


def overlap(x, y):
    return torch.tensor([len(set(r.tolist()) & set(s.tolist())) for r, s in zip(x, y)], dtype=torch.float32)


def nbytes(*ts):
    return int(sum(t.numel() * t.element_size() for t in ts))


def store_legs(E, n_docs, nlist, out):
    g = torch.Generator(device=dev).manual_seed(4141)
    tokens, begin, end = make_store(n_docs, E, g)
    T = tokens.shape[0]
    codes, scales = ops.fp8_quantize_rows(tokens)
    del tokens
    torch.cuda.empty_cache()
    only = TokenStore(None, list(range(n_docs)), begin.cpu().numpy(), end.cpu().numpy(), codes=codes, scales=scales,
                      source_dtype=torch.float16)
    ix = only.build_token_index({"faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": 16}, subsample=a.subsample)
    deq = ops.fp8_dequantize_rows(ix.codes, ix.scales, torch.float16)      # the 16-bit lists an IVFFlatIPIndexer would hold
    lens = torch.diff(ix.list_begin)
    index_common = nbytes(ix.ids, ix.list_begin, ix.centroids)
    out["resident"].append({
        "E": E, "rows": T, "nlist": nlist, "list_rows_max": int(lens.max()), "list_rows_mean": float(lens.float().mean()),
        "fp16_store_plus_16bit_index": T * E * 2 + nbytes(deq) + index_common,
        "fp8_store_plus_16bit_index": nbytes(codes, scales) + nbytes(deq) + index_common,
        "fp8_store_plus_fp8_index": nbytes(codes, scales) + nbytes(ix.codes, ix.scales) + index_common,
        "ids_and_tables": index_common})
    for nq in (32, 2048):
        q = unit_rows(nq, E, g)
        flat = {}
        for k in (128, 512):
            fl = lambda: ops.dot_topk_fp8(q, codes, scales, k)             # noqa: E731
            flat[k] = (bench.gpu_time_ms(fl, a.steps), fl()[1])
        for nprobe in (16, 64):
            probes = ops.dot_topk(q, ix.centroids, nprobe)[1].to(torch.int32)
            for k in (128, 512):
                f8 = lambda: ops.ivf_scan_fp8(q, ix.codes, ix.scales, ix.list_begin, probes, k)     # noqa: E731
                f16 = lambda: ops.ivf_scan(q, deq, ix.list_begin, probes, k)                        # noqa: E731
                t8, t16 = [], []
                for _ in range(2):                                 # alternated; the first round also warms both code objects
                    t16.append(bench.gpu_time_ms(f16, a.steps))
                    t8.append(bench.gpu_time_ms(f8, a.steps))
                ms8, ms16 = min(t8), min(t16)
                (s8, r8), (s16, r16) = f8(), f16()
                hits = ix._ids_of(r8)
                out["scan"].append({
                    "E": E, "rows": T, "nlist": nlist, "nprobe": nprobe, "query_tokens": nq, "k": k, "fp8_ms": ms8,
                    "fp16_ms": ms16, "fp8_over_fp16": ms8 / ms16, "both_rounds_ms": {"fp8": t8, "fp16": t16},
                    "candidates_per_query_mean": float(lens[probes.long()].sum(dim=1).float().mean()),
                    "same_rows_as_fp16_scan": float(overlap(r8, r16).mean()) / k,
                    "scores_bit_equal_to_fp16_scan": bool(torch.equal(s8, s16)),
                    "flat_fp8_ms": flat[k][0], "fp8_scan_over_flat": ms8 / flat[k][0],
                    "overlap_with_flat_fp8_hits_mean": float(overlap(hits, flat[k][1]).mean()) / k})
    if E == 128:
        e2e = {}
        for nprobe in (16, 64):
            ix.nprobe = nprobe
            for nqs in (1, 64):
                qv = torch.nn.functional.normalize(torch.randn(nqs, Q, E, generator=g, device=dev), dim=-1).half()
                fi = lambda: only.search_device(qv, 1000, 128, index=ix)                  # noqa: E731
                ff = lambda: only.search_device(qv, 1000, 128, token_search="fp8")        # noqa: E731
                di, df = fi()[1], ff()[1]
                e2e[f"nprobe_{nprobe}_queries_{nqs}"] = {
                    "index_ms": bench.gpu_time_ms(fi, a.steps), "flat_fp8_ms": bench.gpu_time_ms(ff, a.steps),
                    "token_top_k": 128, "top_n": 1000, "top10_docs_overlap": float(overlap(di[:, :10], df[:, :10]).mean()) / 10,
                    "top1000_docs_overlap": float(overlap(di, df).mean()) / 1000}
        out["end_to_end"] = e2e
    del codes, scales, deq, ix, only
    torch.cuda.empty_cache()


out = {"scan": [], "resident": []}
store_legs(128, a.docs, 4096, out)
if a.docs768 > 0:
    store_legs(768, a.docs768, 1024, out)
print(json.dumps(out))
