#!/usr/bin/env python
"""Benchmark of the fp8 token search (ops.dot_topk_fp8, TokenStore token_search="fp8" / row_shard=) on one GPU, in one
process.  Synthetic stores of MSMARCO-length passages (tools/bench_colbert_search.py's generator: lengths N(70, 25) clipped to
[8, 180], unit fp16 token vectors).  HIP events in steady state (bench.gpu_time_ms), the two kernels alternated.  Prints ONE
JSON line:

  search[]      (a) per store (dim 128: --docs passages = DESIGN §3.12's store; dim 768: --docs768 passages, about the same
                bytes), per query-token count (32, 2048) and k' (128, 512): fp8_ms = ops.dot_topk_fp8 over the quantised rows,
                fp16_ms = ops.dot_topk over ops.fp8_dequantize_rows of them (the same values), their ratio whatever it is, the
                mean overlap of the two hit lists (the values are equal: anything below k' is a tie order or an error); for the
                32-token legs each kernel's needed bytes and fraction of the 8 TB/s peak, for the 2,048-token legs the FLOP and
                the fraction of the nominal MFMA peak
  sharded       (b) row_shard = 2**20 over a store of --rows-sharded rows (8 M): ms of token_hits(token_search="fp8"), and
                whether the ONE-call search succeeds there or gives up after its re-runs
  fidelity      (c) fp8 hits against the 16-bit hits of the UNQUANTISED rows: mean / minimum overlap at k'
  end_to_end    (d) search_device for 1 and 64 queries on the fp8-ONLY store
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
ap.add_argument("--rows-sharded", type=int, default=8 * 2 ** 20)
ap.add_argument("--steps", type=int, default=10)
a = ap.parse_args()
Q, D = 32, 180
dev = torch.device("cuda:0")
MFMA_PEAK = 2.5e15      # nominal dense 16-bit matrix rate of the part, FLOP/s


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


def search_legs(E, n_docs, out):
    g = torch.Generator(device=dev).manual_seed(4141)
    tokens, begin, end = make_store(n_docs, E, g)
    T = tokens.shape[0]
    codes, scales = ops.fp8_quantize_rows(tokens)
    deq = ops.fp8_dequantize_rows(codes, scales, torch.float16)
    for nq in (32, 2048):
        q = unit_rows(nq, E, g)
        for k in (128, 512):
            f8 = lambda: ops.dot_topk_fp8(q, codes, scales, k)     # noqa: E731
            f16 = lambda: ops.dot_topk(q, deq, k)                  # noqa: E731
            t8, t16 = [], []
            for _ in range(2):                                     # alternated; the first round also warms both code objects
                t16.append(bench.gpu_time_ms(f16, a.steps))
                t8.append(bench.gpu_time_ms(f8, a.steps))
            ms8, ms16 = min(t8), min(t16)
            leg = {"E": E, "rows": T, "query_tokens": nq, "k": k, "fp8_ms": ms8, "fp16_ms": ms16, "fp8_over_fp16": ms8 / ms16,
                   "both_rounds_ms": {"fp8": t8, "fp16": t16},
                   "hit_overlap_mean": float(overlap(f8()[1], f16()[1]).mean())}
            if nq == 32:
                fixed = nq * E * 2 + nq * k * 12
                by8, by16 = T * (E + 4) + fixed, T * E * 2 + fixed
                leg.update(fp8_bytes=by8, fp16_bytes=by16, fp8_frac_of_peak=by8 / (ms8 * 1e-3) / 1e9 / bench.HBM_PEAK_GBS,
                           fp16_frac_of_peak=by16 / (ms16 * 1e-3) / 1e9 / bench.HBM_PEAK_GBS)
            else:
                flop = 2.0 * nq * T * E
                leg.update(flop=flop, fp8_frac_of_mfma_peak=flop / (ms8 * 1e-3) / MFMA_PEAK,
                           fp16_frac_of_mfma_peak=flop / (ms16 * 1e-3) / MFMA_PEAK)
            out["search"].append(leg)
    if E == 128:
        # (c) fidelity against the unquantised rows, and (d) end to end on the fp8-only store
        q = unit_rows(256, E, g)
        fid = {}
        for k in (128, 512):
            ov = overlap(ops.dot_topk_fp8(q, codes, scales, k)[1], ops.dot_topk(q, tokens, k)[1])
            fid[f"k{k}"] = {"overlap_mean": float(ov.mean()), "overlap_min": float(ov.min()), "query_tokens": 256}
        out["fidelity"] = fid
        only = TokenStore(None, list(range(n_docs)), begin.cpu().numpy(), end.cpu().numpy(), codes=codes, scales=scales,
                          source_dtype=torch.float16)
        e2e = {}
        for nqs in (1, 64):
            qv = torch.nn.functional.normalize(torch.randn(nqs, Q, E, generator=g, device=dev), dim=-1).half()
            fn = lambda: only.search_device(qv, 1000, 128, token_search="fp8")     # noqa: E731
            e2e[f"queries_{nqs}"] = {"ms": bench.gpu_time_ms(fn, a.steps), "token_top_k": 128, "top_n": 1000}
        out["end_to_end"] = e2e
    del tokens, codes, scales, deq
    torch.cuda.empty_cache()


def sharded_leg(out):
    g = torch.Generator(device=dev).manual_seed(5151)
    T, E, k = a.rows_sharded, 128, 128
    rows = unit_rows(T, E, g)
    codes, scales = ops.fp8_quantize_rows(rows)
    del rows
    torch.cuda.empty_cache()
    st = TokenStore(None, [0], [0], [T], codes=codes, scales=scales, source_dtype=torch.float16)
    qv = torch.nn.functional.normalize(torch.randn(1, Q, E, generator=g, device=dev), dim=-1).half()
    fn = lambda: st.token_hits(qv, k, token_search="fp8", row_shard=2 ** 20)     # noqa: E731
    leg = {"rows": T, "E": E, "query_tokens": Q, "k": k, "row_shard": 2 ** 20, "ms": bench.gpu_time_ms(fn, a.steps)}
    try:
        one = st.token_hits(qv, k, token_search="fp8")
        leg["one_call"] = "succeeds"
        leg["one_call_equals_sharded"] = bool(torch.equal(one, fn()))
        leg["one_call_ms"] = bench.gpu_time_ms(lambda: st.token_hits(qv, k, token_search="fp8"), a.steps)
    except ops.NativeError as e:
        leg["one_call"] = f"fails: {e}"
    out["sharded"] = leg


out = {"hbm_peak_GBps": bench.HBM_PEAK_GBS, "mfma_peak_flops": MFMA_PEAK, "search": []}
search_legs(128, a.docs, out)
if a.docs768 > 0:
    search_legs(768, a.docs768, out)
if a.rows_sharded > 0:
    sharded_leg(out)
print(json.dumps(out))
