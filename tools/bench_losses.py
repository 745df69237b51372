#!/usr/bin/env python
"""Benchmark of the native training losses (matchmaker_amd.losses over mm_pair_loss_fwd / mm_list_loss_fwd) on one
GPU, in one process, on synthetic data.  Every leg is forward + backward of one loss module (zero the gradient, loss, backward
into the leaf scores) on its native route against the module's own eager formula (`native = False`), alternated for two rounds;
the time is the median per-call HIP-event interval in steady state (bench.gpu_time_ms), which for these host-bound chains is what
the loop waits for.  Prints ONE JSON line:

  pairs[]   every pairwise kind at n = 32, 64, 992 (32 x 31, in-batch) and 65,280 (256 x 255)
  lists[]   every list kind at 32 x 64, 64 x 128 (in-batch: B x 2B), 256 x 512 and 32 x 10 (list training)
  step[]    the 64-pair ColBERT training step (ColBERT._score of positives and negatives -> loss -> backward into the bf16
            token vectors) with the eager and the native margin-mse, and the same with a lambdarank in-batch list loss added
  defaults  per kind: native is True only if its slowest native round beats the fastest eager round in EVERY leg of the kind
Every leg is printed, losers included.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import losses  # noqa: E402
from matchmaker_amd.colbert import ColBERT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
a = ap.parse_args()
dev = torch.device("cuda:0")
PAIR_N = [32, 65] if a.small else [32, 64, 992, 65280]
LIST_SHAPES = [(4, 10), (3, 70)] if a.small else [(32, 64), (64, 128), (256, 512), (32, 10)]
PAIR = {"ranknet": losses.RankNetLoss, "margin": losses.MarginRankingLoss1, "margin_mse": losses.MSMarginLoss,
        "mse_pointwise": losses.MSETeacherPointwise, "kldiv_pointwise": losses.KLDivTeacherPointwise,
        "ranknet_teacher": losses.RankNetTeacher, "mse_ranknet": losses.MSERanknetTeacher}
LIST = {"listnet": losses.ListNetLoss, "kldiv": losses.KLDivTeacherList, "smooth_mrr": losses.SmoothMRRLoss,
        "lambda_ndcg2": lambda: losses.LambdaLoss("ndcgLoss2_scheme"),
        "lambda_ndcg2_teacher": lambda: losses.LambdaLossTeacher("ndcgLoss2_scheme")}


def timed(make_step):
    """{native, eager} -> [round 1 us, round 2 us], alternated (the first round also warms)"""
    steps = {native: make_step(native) for native in (True, False)}
    out = {True: [], False: []}
    for _ in range(2):
        for native in (True, False):
            out[native].append(1e3 * bench.gpu_time_ms(steps[native], a.steps, timed_ms=15.0, warm_ms=20.0, max_calls=200))
    return {"native_us": out[True], "eager_us": out[False], "eager_over_native": min(out[False]) / min(out[True]),
            "native_faster": max(out[True]) < min(out[False])}


def loss_step(make_mod, leaves, labels):
    def make(native):
        mod = make_mod().to(dev)
        mod.native = native

        def step():
            for t in leaves:
                t.grad = None
            mod(*leaves, *labels).backward()
        return step
    return make


def pair_leg(kind, n):
    g = torch.Generator(device=dev).manual_seed(n)
    pos, neg = (2 * torch.randn(n, generator=g, device=dev) for _ in range(2))
    if kind == "ranknet":
        labels = [torch.rand(n, generator=g, device=dev)]
    elif kind == "margin":
        labels = [torch.ones(n, device=dev)]
    else:
        labels = [torch.randn(n, generator=g, device=dev).abs() + 0.1 for _ in range(2)]
    return {"kind": kind, "n": n, **timed(loss_step(PAIR[kind], [pos.requires_grad_(), neg.requires_grad_()], labels))}


def list_leg(kind, B, L):
    g = torch.Generator(device=dev).manual_seed(B * L)
    scores = (2 * torch.randn(B, L, generator=g, device=dev)).requires_grad_()
    if kind == "lambda_ndcg2":
        labels = torch.randint(0, 4, (B, L), generator=g, device=dev).float()
    elif kind == "smooth_mrr":
        labels = (torch.rand(B, L, generator=g, device=dev) < 0.2).float()
    else:
        labels = 3 * torch.randn(B, L, generator=g, device=dev)
    return {"kind": kind, "B": B, "L": L, **timed(loss_step(LIST[kind], [scores], [labels]))}


def step_legs():
    B, Q, D, E = (8, 8, 20, 128) if a.small else (64, 32, 180, 128)
    g = torch.Generator(device=dev).manual_seed(64)
    unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, generator=g, device=dev), dim=-1).bfloat16().requires_grad_()  # noqa: E731
    q, dp, dn = unit(B, Q, E), unit(B, D, E), unit(B, D, E)
    qm = torch.ones(B, Q, dtype=torch.int64, device=dev)
    dm = torch.ones(B, D, dtype=torch.int64, device=dev)
    tp, tn = (3 * torch.randn(B, generator=g, device=dev) for _ in range(2))
    # the in-batch list of train.py:446-450: [B, 2B] scores of every query against every positive and negative document
    qv, dv = unit(B // 2, E), unit(B, E)
    teacher = 3 * torch.randn(B // 2, B, generator=g, device=dev)
    out = []
    for name, inbatch in (("colbert_64_pairs_margin_mse", False), ("colbert_64_pairs_margin_mse_plus_inbatch_lambdarank", True)):
        def make(native, inbatch=inbatch):
            main, ib = losses.MSMarginLoss(), losses.LambdaLossTeacher("ndcgLoss2_scheme")
            main.native = ib.native = native

            def step():
                for t in (q, dp, dn, qv, dv):
                    t.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16):      # train.py:347-409: forward and loss under autocast
                    loss = main(ColBERT._score(q, dp, qm, dm), ColBERT._score(q, dn, qm, dm), tp, tn)
                    if inbatch:
                        loss = loss + ib(torch.mm(qv, dv.t()).float(), teacher)
                loss.backward()
            return step
        out.append({"step": name, "pairs": B, **timed(make)})
    return out


pair_leg("margin_mse", PAIR_N[0]), list_leg("listnet", *LIST_SHAPES[0])      # the process's first seconds (clocks, allocator, first
#                                                                               launches) belong to no leg: the first kind measured
#                                                                               came out bimodal (98 / 61 us) without this
out = {"pairs": [pair_leg(k, n) for k in PAIR for n in PAIR_N], "lists": [list_leg(k, B, L) for k in LIST for B, L in LIST_SHAPES],
       "step": step_legs()}
out["defaults"] = {k: all(r["native_faster"] for r in out["pairs"] + out["lists"] if r["kind"] == k) for k in list(PAIR) + list(LIST)}
out["what"] = "us per forward + backward, median HIP-event interval in steady state, [round 1, round 2]"
print(json.dumps(out))
