#!/usr/bin/env python
"""Benchmark of the fused DRMM kernel (mm_drmm_fwd) at the reference shape (Q 30, D 200, E 300, 10 bins; models/all.py:154)
on one GPU.  Prints ONE JSON line:

  hist_shared / hist_replicated   64 queries x 1000 candidates, histograms out, query tile shared / one copy per pair
  score_shared                    the same call with the head fused (inference), against hist + the torch head
  eval_512                        an eval.py-sized call: 512 pairs, pair-per-row
  train_64                        a training step of 64 pairs through the drop-in (forward + backward + nothing else)
each with ms, M pairs/s, the fraction of HBM peak (8 TB/s) and of the box's calibrated stream (ops.hbm_stream_probe over the
document tensor) that the document bytes represent, and the ratio to two eager baselines on the same GPU:
  literal   the reference's own path: GPU cosine, .cpu(), torch.histc per (pair, query token), copy back (512 pairs only)
  device    a fair device-only torch version: bmm, bin index, scatter_add_
and to ops.kernel_pool with KNRM's 11 kernels on the same tensors (MM_KP_F32MFMA=1 in the environment selects its
exact-fp32 twin; the JSON says which ran).  Timing: bench.gpu_time_ms (median of per-call HIP events in steady state)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops  # noqa: E402
from matchmaker_amd.drmm import DRMM  # noqa: E402
from matchmaker_amd.knrm import kernel_mus, kernel_sigmas  # noqa: E402

HBM_PEAK_GBPS = 8000.0

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--cands", type=int, default=1000)
ap.add_argument("--eager-queries", type=int, default=8, help="queries of the device-only eager legs (scaled per pair)")
a = ap.parse_args()
dev = torch.device("cuda:0")
Q, D, E, BINS = 30, 200, 300, 10


class VecEmbedder(torch.nn.Module):
    def get_output_dim(self):
        return E

    def forward(self, t):
        return t["vecs"]


torch.manual_seed(0)
m = DRMM(VecEmbedder(), BINS).to(dev)
l0, l1 = m.matching_classifier._linear_layers
g = torch.Generator(device=dev).manual_seed(1)
nq, B = a.queries, a.queries * a.cands
q = torch.randn(nq, Q, E, generator=g, device=dev)
d = torch.randn(B, D, E, generator=g, device=dev)
q_rep = q.repeat_interleave(a.cands, dim=0)
gate = torch.softmax(torch.randn(nq, Q, generator=g, device=dev), dim=-1)


def cosine(qq, dd):
    qn = qq / (qq.norm(p=2, dim=-1, keepdim=True) + 1e-13)
    dn = dd / (dd.norm(p=2, dim=-1, keepdim=True) + 1e-13)
    return torch.bmm(qn, dn.transpose(-1, -2))


def eager_device(qq, dd):
    """histc's rule with device ops only: bin index + scatter_add_."""
    c = cosine(qq, dd)
    inr = ((c >= -1) & (c <= 1)).float()
    b = ((c + 1) / 2 * BINS).long().clamp_(0, BINS - 1)
    return torch.zeros(c.shape[0], c.shape[1], BINS, device=c.device).scatter_add_(-1, b, inr)


def eager_literal(qq, dd):
    """drmm.py:66-76 as written."""
    c = cosine(qq, dd).cpu()
    h = torch.empty((c.shape[0], c.shape[1], BINS))
    for b in range(c.shape[0]):
        for i in range(c.shape[1]):
            h[b, i] = torch.histc(c[b, i], bins=BINS, min=-1, max=1)
    return h.to(qq.device)


def head(h, gates):
    return torch.sum(m.matching_classifier(torch.log1p(h)) * gates.unsqueeze(-1), dim=1)


def leg(name, ms, pairs, **extra):
    gbs = pairs * D * E * 4 / ms / 1e6
    r = {"ms": ms, "M_pairs_per_s": pairs / ms / 1e3, "doc_GBps": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBPS,
         "frac_of_calibrated": gbs / stream_gbs}
    r.update(extra)
    out[name] = r


out = {"shape": {"Q": Q, "D": D, "E": E, "bins": BINS, "queries": nq, "cands": a.cands},
       "kernel_pool_variant": "exact-fp32 MFMA (MM_KP_F32MFMA=1)" if os.environ.get("MM_KP_F32MFMA") == "1" else "split-bf16 (default)"}
mu = torch.tensor(kernel_mus(11), device=dev)
sigma = torch.tensor(kernel_sigmas(11), device=dev)
ones11 = torch.ones(11, device=dev)
with torch.no_grad():
    probe_ms = bench.gpu_time_ms(lambda: ops.hbm_stream_probe(d), a.steps)
    stream_gbs = (d.numel() * 4) // 8192 * 8192 / probe_ms / 1e6
    out["calibrated_stream_GBps"] = stream_gbs
    ne = a.eager_queries * a.cands
    dev_ms = bench.gpu_time_ms(lambda: eager_device(q_rep[:ne], d[:ne]), max(2, a.steps // 3)) / ne
    kp_s = bench.gpu_time_ms(lambda: ops.kernel_pool(q, d, None, None, mu, sigma, ones11, ones11, a.cands), a.steps)
    kp_r = bench.gpu_time_ms(lambda: ops.kernel_pool(q_rep, d, None, None, mu, sigma, ones11, ones11, 1), a.steps)
    t = bench.gpu_time_ms(lambda: ops.drmm_hist(q, d, BINS, a.cands), a.steps)
    leg("hist_shared", t, B, eager_device_ms=dev_ms * B, speedup_vs_eager_device=dev_ms * B / t, kernel_pool_ms=kp_s,
        ratio_to_kernel_pool=t / kp_s)
    t = bench.gpu_time_ms(lambda: ops.drmm_hist(q_rep, d, BINS, 1), a.steps)
    leg("hist_replicated", t, B, eager_device_ms=dev_ms * B, speedup_vs_eager_device=dev_ms * B / t, kernel_pool_ms=kp_r,
        ratio_to_kernel_pool=t / kp_r)
    gates_rep = gate.repeat_interleave(a.cands, dim=0)
    t_f = bench.gpu_time_ms(lambda: ops.drmm_score(q, d, gate, l0.weight, l0.bias, l1.weight, l1.bias, a.cands), a.steps)
    t_h = bench.gpu_time_ms(lambda: head(ops.drmm_hist(q, d, BINS, a.cands), gates_rep), a.steps)
    leg("score_shared", t_f, B, hist_plus_torch_head_ms=t_h, fused_saves_ms=t_h - t_f)
    e512 = bench.gpu_time_ms(lambda: eager_device(q_rep[:512], d[:512]), a.steps)
    lit = bench.gpu_time_ms(lambda: eager_literal(q_rep[:512], d[:512]), 2, warmup=1, warm_ms=0.0, timed_ms=0.0)
    kp5 = bench.gpu_time_ms(lambda: ops.kernel_pool(q_rep[:512], d[:512], None, None, mu, sigma, ones11, ones11, 1), a.steps)
    t = bench.gpu_time_ms(lambda: ops.drmm_hist(q_rep[:512], d[:512], BINS, 1), a.steps)
    leg("eval_512", t, 512, eager_device_ms=e512, speedup_vs_eager_device=e512 / t, eager_literal_ms=lit,
        speedup_vs_eager_literal=lit / t, kernel_pool_ms=kp5, ratio_to_kernel_pool=t / kp5)

m.train()
tok_q = torch.full((64, Q), 5, device=dev)
tok_d = torch.full((64, D), 5, device=dev)
qt, dt = q_rep[:64].clone(), d[:64].clone()


def train_native():
    m.zero_grad(set_to_none=True)
    m({"tokens": tok_q, "vecs": qt}, {"tokens": tok_d, "vecs": dt}).sum().backward()


def train_eager():
    m.zero_grad(set_to_none=True)
    gates = m.query_softmax(m.query_gate(qt).squeeze(-1), torch.ones(64, Q, device=dev))
    head(eager_device(qt, dt), gates).sum().backward()


t_n, t_e = bench.gpu_time_ms(train_native, a.steps), bench.gpu_time_ms(train_eager, a.steps)
leg("train_64", t_n, 64, eager_device_ms=t_e, speedup_vs_eager_device=t_e / t_n)
out["note"] = (f"document bytes {B * D * E * 4 / 1e9:.2f} GB per {nq}x{a.cands} call; device-only eager legs timed on {ne} "
               f"pairs and scaled per pair; the literal path on 512 pairs")
print(json.dumps(out))
