#!/usr/bin/env python
"""Benchmark of the native in-batch negatives (matchmaker_amd.inbatch over mm_inbatch_dot_loss_fwd / mm_inbatch_select_loss_fwd,
DESIGN §3.24) on one GPU, in one process, on synthetic data.  Every leg is forward + backward from leaf vectors to their
gradients (zero the gradients, the paired score sp = <q_i, dp_i>, InBatchNegatives, backward) on the native route against the
module's own eager formula (`native=False`: the torch chain of train.py:434-472), alternated for two rounds; the time is the
median per-call HIP-event interval in steady state (bench.gpu_time_ms).  fp16 legs run under autocast, as train.py does.
Prints ONE JSON line:

  pair[]     Margin-MSE with teacher and RankNet without, B in {32, 64, 128, 256} x E in {128, 768}, fp16 and fp32
  list[]     KLDivTeacherList and LambdaLossTeacher at B in {32, 128}, E = 768, fp16 and fp32
  colbert[]  maxsim_inbatch -> forward_scores -> backward into the bf16 token vectors at 32 x 32, Margin-MSE and KLDivTeacherList
  defaults   per family: native is True only if its slowest native round beats the fastest eager round in EVERY leg
Every leg is printed, losers included.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import matchmaker_amd.torch_ops  # noqa: E402,F401
from matchmaker_amd import inbatch, losses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
a = ap.parse_args()
dev = torch.device("cuda:0")
PAIR_B, PAIR_E = ([8, 33], [16]) if a.small else ([32, 64, 128, 256], [128, 768])
LIST_B = [8] if a.small else [32, 128]
LOSS = {"margin_mse": (losses.MSMarginLoss, False, True), "ranknet": (losses.RankNetLoss, False, False),
        "kldiv_list": (losses.KLDivTeacherList, True, True),
        "lambda_teacher": (lambda: losses.LambdaLossTeacher("ndcgLoss2_scheme"), True, True)}


def timed(make_step):
    """{native, eager} -> [round 1 us, round 2 us], alternated (the first round also warms)"""
    steps = {native: make_step(native) for native in (True, False)}
    out = {True: [], False: []}
    for _ in range(2):
        for native in (True, False):
            out[native].append(1e3 * bench.gpu_time_ms(steps[native], a.steps, timed_ms=15.0, warm_ms=20.0, max_calls=200))
    return {"native_us": out[True], "eager_us": out[False], "eager_over_native": min(out[False]) / min(out[True]),
            "native_faster": max(out[True]) < min(out[False])}


def dot_leg(kind, B, E, dtype):
    make_loss, use_list, teacher = LOSS[kind]
    g = torch.Generator(device=dev).manual_seed(B * E)
    Q, Dp, Dn = ((torch.randn(B, E, generator=g, device=dev) / E ** 0.25).requires_grad_() for _ in range(3))
    Tp, Tn = ((3 * torch.randn(B, B, generator=g, device=dev)) if teacher else None for _ in range(2))

    def make(native):
        mod = inbatch.InBatchNegatives(make_loss().to(dev), use_list, native=native)

        def step():
            for t in (Q, Dp, Dn):
                t.grad = None
            with torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16):
                q, dp, dn = (t.to(dtype) for t in (Q, Dp, Dn))      # (fp32: no-ops)
                sp = (q * dp).sum(-1)
                if native:
                    assert mod.dot_route(sp, q, dp, dn, Tp, Tn)
                loss, _ = mod(sp, q, dp, dn, Tp, Tn)
            loss.backward()
        return step
    return {"kind": kind, "B": B, "E": E, "dtype": str(dtype).replace("torch.", ""), **timed(make)}


def colbert_leg(kind):
    make_loss, use_list, teacher = LOSS[kind]
    B, Qn, Dn_, E = (8, 8, 20, 128) if a.small else (32, 32, 180, 128)
    g = torch.Generator(device=dev).manual_seed(32)
    unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, generator=g, device=dev), dim=-1).bfloat16().requires_grad_()  # noqa: E731
    q, dp, dn = unit(B, Qn, E), unit(B, Dn_, E), unit(B, Dn_, E)
    Tp, Tn = (3 * torch.randn(B, B, generator=g, device=dev) for _ in range(2))

    def make(native):
        mod = inbatch.InBatchNegatives(make_loss().to(dev), use_list, native=native)

        def step():
            for t in (q, dp, dn):
                t.grad = None
            Sp = torch.ops.mm_native.maxsim_inbatch(q, None, dp, None)
            Sn = torch.ops.mm_native.maxsim_inbatch(q, None, dn, None)
            loss, _ = mod.forward_scores(Sp.diagonal(), Sp, Sn, Tp, Tn)
            loss.backward()
        return step
    return {"kind": kind, "B": B, "Q": Qn, "D": Dn_, "E": E, **timed(make)}


dot_leg("margin_mse", PAIR_B[0], PAIR_E[0], torch.float32)      # the process's first seconds (clocks, allocator, first launches)
#                                                                  belong to no leg
out = {"pair": [dot_leg(k, B, E, dt) for k in ("margin_mse", "ranknet") for dt in (torch.float16, torch.float32) for E in PAIR_E for B in PAIR_B],
       "list": [dot_leg(k, B, PAIR_E[-1], dt) for k in ("kldiv_list", "lambda_teacher") for dt in (torch.float16, torch.float32) for B in LIST_B],
       "colbert": [colbert_leg(k) for k in ("margin_mse", "kldiv_list")]}
out["defaults"] = {"pair": all(r["native_faster"] for r in out["pair"] + out["colbert"][:1]),
                   "list": all(r["native_faster"] for r in out["list"] + out["colbert"][1:])}
out["what"] = "us per forward + backward, median HIP-event interval in steady state, [round 1, round 2]"
print(json.dumps(out))
