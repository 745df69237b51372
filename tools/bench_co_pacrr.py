#!/usr/bin/env python
"""Benchmark of the fused CO-PACRR kernels (mm_co_pacrr_fwd / mm_co_pacrr_bwd) at the reference config (Q 30, U = D 200,
E 300, C 32, N 3, k 5; config/train/non-bert-defaults.yaml:54-58) against the module's own eager path (allennlp cosine, the
nn.Sequential(ConstantPad2d, Conv2d, MaxPool3d) blocks, doc_context_pool, torch.topk per view and index_select of the
contexts) on the same GPU, and against PACRR's fused forward (mm_pacrr_fwd) on the same inputs.  Prints ONE JSON line:

  fwd_shared      64 queries x 1000 candidates, query tile shared (pairs_per_query = 1000)
  fwd_replicated  the same pairs in the reference's layout (one query copy per pair)
  eval_512        an eval.py-sized call: 512 pairs, pair-per-row (batch_size_eval, config/train/defaults.yaml:115)
  train_64        a training step of 64 pairs: forward with saved positions + backward (grad_out = ones)
each with ms, M pairs/s, the fraction of HBM peak (8 TB/s) and of the box's calibrated stream (ops.hbm_stream_probe over the
document tensor) that the document bytes represent, the speedup over eager and the time relative to PACRR's native call
(forward legs: mm_pacrr_fwd; training: mm_pacrr_fwd + mm_pacrr_bwd).  Timing: bench.gpu_time_ms (median of
per-call HIP events in steady state)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops  # noqa: E402
from matchmaker_amd.co_pacrr import CO_PACRR  # noqa: E402
from tests import co_pacrr_reference as CP  # noqa: E402

HBM_PEAK_GBPS = 8000.0

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--cands", type=int, default=1000)
ap.add_argument("--eager-queries", type=int, default=4, help="queries of the eager legs (its [B, 32, Q, D] tensors are large)")
a = ap.parse_args()
dev = torch.device("cuda:0")
Q, D, E, N, C, k = 30, 200, 300, 3, 32, 5
torch.manual_seed(0)
m = CO_PACRR(Q, D, N, C, k).to(dev).eval()
views = m.kmax_pooling_views
ws, bs = m._conv_params()
g = torch.Generator(device=dev).manual_seed(1)
nq, B = a.queries, a.queries * a.cands
q = torch.randn(nq, Q, E, generator=g, device=dev)
d = torch.randn(B, D, E, generator=g, device=dev)
q_rep = q.repeat_interleave(a.cands, dim=0)


def eager(qq, dd):
    """The reference's forward up to per_query_results (co_pacrr.py:90-158) through the module's own modules + torch.topk
    (tests/test_co_pacrr_gpu.py restates the same graph)."""
    cos = CP.cosine(qq, dd)[:, None]
    ctx = CP.cosine(qq.mean(dim=1, keepdim=True), m.doc_context_pool(dd.transpose(1, 2)).transpose(1, 2))[:, 0]
    out = []
    for path in [cos] + [conv(cos) for conv in m.convolutions]:
        vals, cols = [], []
        for v in views:
            val, c = torch.topk(path.squeeze(1)[:, :, 0:v], k=k, sorted=True)
            vals.append(val)
            cols.append(c)
        c = torch.cat(cols, dim=-1)
        out.append(torch.cat(vals + [torch.gather(ctx[:, None].expand(-1, c.shape[1], -1), -1, c)], dim=-1))
    return torch.cat(out, dim=-1)


def leg(name, ms, pairs, eager_ms_per_pair=None, pacrr_ms=None):
    gbs = pairs * D * E * 4 / ms / 1e6
    r = {"ms": ms, "M_pairs_per_s": pairs / ms / 1e3, "doc_GBps": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBPS,
         "frac_of_calibrated": gbs / stream_gbs}
    if eager_ms_per_pair is not None:
        r["eager_ms"] = eager_ms_per_pair * pairs
        r["speedup_vs_eager"] = eager_ms_per_pair * pairs / ms
    if pacrr_ms is not None:
        r["pacrr_native_ms"] = pacrr_ms
        r["ratio_to_pacrr_native"] = ms / pacrr_ms
    out[name] = r


out = {"shape": {"Q": Q, "D": D, "E": E, "C": C, "N": N, "k": k, "queries": nq, "cands": a.cands}}
with torch.no_grad():
    probe_ms = bench.gpu_time_ms(lambda: ops.hbm_stream_probe(d), a.steps)
    stream_gbs = (d.numel() * 4) // 8192 * 8192 / probe_ms / 1e6
    out["calibrated_stream_GBps"] = stream_gbs
    ne = a.eager_queries * a.cands
    e_ms = bench.gpu_time_ms(lambda: eager(q_rep[:ne], d[:ne]), max(2, a.steps // 3)) / ne
    leg("fwd_shared", bench.gpu_time_ms(lambda: ops.co_pacrr_kmax(q, d, ws, bs, k, views, a.cands), a.steps), B, e_ms,
        bench.gpu_time_ms(lambda: ops.pacrr_kmax(q, d, ws, bs, k, a.cands), a.steps))
    leg("fwd_replicated", bench.gpu_time_ms(lambda: ops.co_pacrr_kmax(q_rep, d, ws, bs, k, views, 1), a.steps), B, e_ms,
        bench.gpu_time_ms(lambda: ops.pacrr_kmax(q_rep, d, ws, bs, k, 1), a.steps))
    e512 = bench.gpu_time_ms(lambda: eager(q_rep[:512], d[:512]), a.steps) / 512
    leg("eval_512", bench.gpu_time_ms(lambda: ops.co_pacrr_kmax(q_rep[:512], d[:512], ws, bs, k, views, 1), a.steps), 512,
        e512, bench.gpu_time_ms(lambda: ops.pacrr_kmax(q_rep[:512], d[:512], ws, bs, k, 1), a.steps))
qt, dt = q_rep[:64].clone(), d[:64].clone()


def train_native():
    o, idx = ops.co_pacrr_kmax(qt, dt, ws, bs, k, views, 1, save=True)
    return ops.co_pacrr_kmax_bwd(qt, dt, ws, idx, torch.ones_like(o), k, views)


def train_pacrr():
    o, idx = ops.pacrr_kmax(qt, dt, ws, bs, k, 1, save=True)
    return ops.pacrr_kmax_bwd(qt, dt, ws, idx, torch.ones_like(o), k)


def train_eager():
    qq, dd = qt.clone().requires_grad_(True), dt.clone().requires_grad_(True)
    eager(qq, dd).sum().backward()


leg("train_64", bench.gpu_time_ms(train_native, a.steps), 64, bench.gpu_time_ms(train_eager, a.steps) / 64,
    bench.gpu_time_ms(train_pacrr, a.steps))
d_bytes = B * D * E * 4
out["note"] = (f"document bytes {d_bytes / 1e9:.2f} GB per 64x1000 call; eager legs timed on {ne} pairs and scaled per pair")
print(json.dumps(out))
