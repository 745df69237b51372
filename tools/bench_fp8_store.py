#!/usr/bin/env python
"""Benchmark of the fp8 ColBERT token store on one GPU, in one process.  Synthetic stores of MSMARCO-length passages (the
generator of bench.py's ragged-aggregate leg: lengths N(70, 25) clipped to [8, 180], unit fp16 token vectors), Q 32.
Prints ONE JSON line:

  aggregate[]   per dim (128: bench.py's extra_ragged_aggregate shape, a store of 2 M passages; 768: as many passages as
                --docs768 says), 64 queries x 1000 random candidates in one launch, the two kernels alternated:
                  fp16_ms / fp8_ms     median per-call HIP-event time in steady state (bench.gpu_time_ms) of ops.maxsim_ragged
                                       over the fp16 store and ops.maxsim_ragged_fp8 over its quantisation, same candidates
                  fp8_over_fp16        the ratio of the two times (< 1: fp8 faster), whatever it is
                  *_bytes, *_GBps, *_frac_of_peak   the bytes each kernel needs (rows x row bytes [+ 4 B of scale per row] +
                                       queries + ranges + scores), its rate on them and that rate over the 8 TB/s HBM peak
                  stream_GBps          mm_hbm_stream_probe over the fp16 store: what this box gives the 16-bit kernel's stream
  quantiser     ops.fp8_quantize_rows over the dim-128 store: ms, GB/s of INPUT read, GB/s of input + output, and the input
                rate over the calibrated read stream
  fidelity      fp8 against fp16 scores (both with fp16-rounded maxima, as the searcher head scores) of --fid-nq queries x
                --fid-cands random candidates: the largest |score change|, mean and sigma of the fp16 scores, and the mean /
                minimum overlap of the top-10 / top-100 / top-1000 per query
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=2_000_000, help="passages of the dim-128 store (bench.py: 2 M = 36 GB fp16)")
ap.add_argument("--docs768", type=int, default=300_000, help="passages of the dim-768 store (300 k = 32 GB fp16)")
ap.add_argument("--nq", type=int, default=64)
ap.add_argument("--cands", type=int, default=1000)
ap.add_argument("--fid-nq", type=int, default=16)
ap.add_argument("--fid-cands", type=int, default=5000)
ap.add_argument("--steps", type=int, default=20)
a = ap.parse_args()
Q, D = 32, 180
dev = torch.device("cuda:0")
PEAK = bench.HBM_PEAK_GBS


def make_store(n_docs, E, g):
    lens = synth.msmarco_doc_lengths(n_docs, D, g, dev).long()
    end = torch.cumsum(lens, 0)
    begin = end - lens
    T = int(end[-1])
    tokens = torch.empty((T, E), dtype=torch.float16, device=dev)
    step = (1 << 31) // E
    for s0 in range(0, T, step):
        n = min(step, T - s0)
        tokens[s0:s0 + n] = torch.nn.functional.normalize(torch.randn(n, E, generator=g, device=dev), dim=-1).half()
    return tokens, begin, end, T


def aggregate_leg(E, n_docs, out):
    g = torch.Generator(device=dev).manual_seed(3131)
    tokens, begin, end, T = make_store(n_docs, E, g)
    q = torch.nn.functional.normalize(torch.randn(a.nq, Q, E, generator=g, device=dev), dim=-1).half()
    cand = torch.randint(0, n_docs, (a.nq, a.cands), generator=g, device=dev)
    bb, ee = begin[cand].reshape(-1).contiguous(), end[cand].reshape(-1).contiguous()
    codes, scales = ops.fp8_quantize_rows(tokens)
    f16 = lambda: ops.maxsim_ragged(q, tokens, bb, ee, None, pairs_per_query=a.cands, check_ranges=False, sim_round=True)
    f8 = lambda: ops.maxsim_ragged_fp8(q, codes, scales, bb, ee, None, pairs_per_query=a.cands, check_ranges=False, sim_round=True)
    # alternated, two rounds each: the first round also warms both code objects
    t16, t8 = [], []
    for _ in range(2):
        t16.append(bench.gpu_time_ms(f16, a.steps))
        t8.append(bench.gpu_time_ms(f8, a.steps))
    ms16, ms8 = min(t16), min(t8)
    rows = int((ee - bb).sum())
    fixed = a.nq * Q * E * 2 + 16 * a.nq * a.cands + 4 * a.nq * a.cands
    by16, by8 = rows * E * 2 + fixed, rows * (E + 4) + fixed
    probe_ms = bench.gpu_time_ms(lambda: ops.hbm_stream_probe(tokens, nt=True), 5)
    stream = (tokens.numel() * 2 // 8192 * 8192) / (probe_ms * 1e-3) / 1e9
    leg = {"E": E, "store": f"{n_docs} passages, {T} token rows, {T * E * 2 / 1e9:.1f} GB fp16 / {T * (E + 4) / 1e9:.1f} GB fp8",
           "pairs": a.nq * a.cands, "candidate_rows": rows, "fp16_ms": ms16, "fp8_ms": ms8, "fp8_over_fp16": ms8 / ms16,
           "both_rounds_ms": {"fp16": t16, "fp8": t8},
           "fp16_bytes": by16, "fp8_bytes": by8, "fp16_GBps": by16 / (ms16 * 1e-3) / 1e9, "fp8_GBps": by8 / (ms8 * 1e-3) / 1e9,
           "stream_GBps": stream}
    leg["fp16_frac_of_peak"] = leg["fp16_GBps"] / PEAK
    leg["fp8_frac_of_peak"] = leg["fp8_GBps"] / PEAK
    out["aggregate"].append(leg)
    if E == 128:
        qms = bench.gpu_time_ms(lambda: ops.fp8_quantize_rows(tokens), 5)
        inb = tokens.numel() * 2
        out["quantiser"] = {"rows": T, "E": E, "ms": qms, "input_GBps": inb / (qms * 1e-3) / 1e9,
                            "input_plus_output_GBps": (inb + T * (E + 4)) / (qms * 1e-3) / 1e9,
                            "input_over_read_stream": inb / (qms * 1e-3) / 1e9 / stream, "read_stream_GBps": stream}
        # rank fidelity on this store
        qf = torch.nn.functional.normalize(torch.randn(a.fid_nq, Q, E, generator=g, device=dev), dim=-1).half()
        cf = torch.stack([torch.randperm(n_docs, generator=g, device=dev)[: a.fid_cands] for _ in range(a.fid_nq)])
        fb, fe = begin[cf].reshape(-1).contiguous(), end[cf].reshape(-1).contiguous()
        s16 = ops.maxsim_ragged(qf, tokens, fb, fe, None, pairs_per_query=a.fid_cands, check_ranges=False, sim_round=True).view(a.fid_nq, -1)
        s8 = ops.maxsim_ragged_fp8(qf, codes, scales, fb, fe, None, pairs_per_query=a.fid_cands, check_ranges=False, sim_round=True).view(a.fid_nq, -1)
        fid = {"queries": a.fid_nq, "candidates_per_query": a.fid_cands, "largest_score_change": float((s8 - s16).abs().max()),
               "fp16_score_mean": float(s16.mean()), "fp16_score_sigma": float(s16.std())}
        for k in (10, 100, 1000):
            if k > a.fid_cands:
                continue
            t16k, t8k = s16.topk(k, dim=1).indices, s8.topk(k, dim=1).indices
            ov = torch.tensor([len(set(x.tolist()) & set(y.tolist())) for x, y in zip(t16k, t8k)], dtype=torch.float32)
            fid[f"top{k}_overlap_mean"] = float(ov.mean())
            fid[f"top{k}_overlap_min"] = float(ov.min())
        out["fidelity"] = fid
    del tokens, codes, scales
    torch.cuda.empty_cache()


out = {"Q": Q, "hbm_peak_GBps": PEAK, "aggregate": []}
aggregate_leg(128, a.docs, out)
if a.docs768 > 0:
    aggregate_leg(768, a.docs768, out)
print(json.dumps(out))
