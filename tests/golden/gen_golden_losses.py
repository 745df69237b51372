#!/usr/bin/env python
"""Generates tests/golden/losses_*.npz by driving the REAL reference loss classes (matchmaker/losses/*.py) on CPU fp32
tensors: inputs, loss and the autograd gradients with respect to the scores.  Data only.  Needs the reference tree
(oracle.ref_harness.REFERENCE_ROOT), so it runs in the build container only; the tests read the files.

    python tests/golden/gen_golden_losses.py

losses_pairs.npz   pos, neg, a (labels >= 0, so KLDiv is finite), b, y01 (targets in [0, 1]), ysign (+-1), n = 65; per kind
                   <kind>.loss / .gpos / .gneg
losses_lists.npz   two shapes (5 x 17 and 3 x 70: one wavefront / one workgroup per list): scores_<L>, labels_<L> (teacher scores),
                   grades_<L> (integer grades, -1 = padded; one list with some, one with all but one, one fully padded);
                   per kind <kind>_<L>.loss / .grad, and smooth_mrr_<L>.per_list (agg=False);
                   lambda_args_<i>.loss / .grad: LambdaLoss with the i-th (scheme, keywords) of
                   tests/losses_reference.LAMBDA_ARG_CASES on scores_17 / grades_17
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from tests.losses_reference import LAMBDA_ARG_CASES  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def reference_classes():
    if ref_harness.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REFERENCE_ROOT)
    from matchmaker.losses.lambdarank import LambdaLoss, LambdaLossTeacher
    from matchmaker.losses.listnet import ListNetLoss
    from matchmaker.losses.loss_smooth_mrr import SmoothMRRLoss
    from matchmaker.losses.msmargin import MSMarginLoss
    from matchmaker.losses.ranknet import RankNetLoss
    from matchmaker.losses.teacher_kldiv_list import KLDivTeacherList
    from matchmaker.losses.teacher_kldiv_pointwise import KLDivTeacherPointwise
    from matchmaker.losses.teacher_mse_pointwise import MSETeacherPointwise
    from matchmaker.losses.teacher_mse_ranknet import MSERanknetTeacher
    from matchmaker.losses.teacher_ranknetweighted import RankNetTeacher
    return {"ranknet": RankNetLoss, "margin": lambda: torch.nn.MarginRankingLoss(margin=1, reduction="mean"),
            "margin_mse": MSMarginLoss, "mse_pointwise": MSETeacherPointwise, "kldiv_pointwise": KLDivTeacherPointwise,
            "ranknet_teacher": RankNetTeacher, "mse_ranknet": MSERanknetTeacher, "listnet": ListNetLoss,
            "kldiv": KLDivTeacherList, "smooth_mrr": SmoothMRRLoss, "lambda_ndcg2": lambda: LambdaLoss("ndcgLoss2_scheme"),
            "lambda_ndcg2_teacher": lambda: LambdaLossTeacher("ndcgLoss2_scheme")}


def pair_labels(kind, d):
    return {"ranknet": (d["y01"],), "margin": (d["ysign"],)}.get(kind, (d["a"], d["b"]))


def run_pair(cls, pos, neg, labels):
    p, n = torch.from_numpy(pos).requires_grad_(), torch.from_numpy(neg).requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # KLDivLoss's reduction='mean' note
        loss = cls()(p, n, *[torch.from_numpy(t) for t in labels])
    loss.backward()
    return loss.detach().numpy(), p.grad.numpy(), n.grad.numpy()


def run_list(cls, scores, labels, **kw):
    s = torch.from_numpy(scores).requires_grad_()
    loss = cls()(s * 1.0, torch.from_numpy(labels).clone(), **kw)      # (s * 1.0: LambdaLoss writes into its argument in place)
    (loss.sum() if loss.dim() else loss).backward()
    return loss.detach().numpy(), s.grad.numpy()


def make_pairs(rng, n=65):
    f = np.float32
    return {"pos": f(2 * rng.standard_normal(n)), "neg": f(2 * rng.standard_normal(n)), "a": f(np.abs(rng.standard_normal(n)) + 0.1),
            "b": f(np.abs(rng.standard_normal(n)) + 0.1), "y01": f(rng.random(n)), "ysign": f(rng.choice([-1.0, 1.0], n))}


def make_lists(rng, B, L):
    f = np.float32
    grades = f(rng.integers(0, 4, (B, L)))
    grades[0, L // 2:] = -1           # some padded
    grades[1, 1:] = -1                # all but one
    grades[2, :] = -1                 # fully padded: term 0, gradient 0
    return f(2 * rng.standard_normal((B, L))), f(3 * rng.standard_normal((B, L))), grades


def main():
    ref = reference_classes()
    rng = np.random.default_rng(20)
    d = make_pairs(rng)
    out = dict(d)
    for kind in ("ranknet", "margin", "margin_mse", "mse_pointwise", "kldiv_pointwise", "ranknet_teacher", "mse_ranknet"):
        out[kind + ".loss"], out[kind + ".gpos"], out[kind + ".gneg"] = run_pair(ref[kind], d["pos"], d["neg"], pair_labels(kind, d))
    np.savez(os.path.join(OUT, "losses_pairs.npz"), **out)
    out = {}
    for B, L in ((5, 17), (3, 70)):
        scores, labels, grades = make_lists(rng, B, L)
        out[f"scores_{L}"], out[f"labels_{L}"], out[f"grades_{L}"] = scores, labels, grades
        for kind in ("listnet", "kldiv", "lambda_ndcg2_teacher"):
            out[f"{kind}_{L}.loss"], out[f"{kind}_{L}.grad"] = run_list(ref[kind], scores, labels)
        out[f"lambda_ndcg2_{L}.loss"], out[f"lambda_ndcg2_{L}.grad"] = run_list(ref["lambda_ndcg2"], scores, grades)
        mrr_labels = np.float32(np.maximum(grades, 0) > 1)
        out[f"smooth_mrr_{L}.labels"] = mrr_labels
        out[f"smooth_mrr_{L}.loss"], out[f"smooth_mrr_{L}.grad"] = run_list(ref["smooth_mrr"], scores, mrr_labels)
        out[f"smooth_mrr_{L}.per_list"] = run_list(ref["smooth_mrr"], scores, mrr_labels, agg=False)[0]
    from matchmaker.losses.lambdarank import LambdaLoss
    for i, (scheme, kw) in enumerate(LAMBDA_ARG_CASES):
        out[f"lambda_args_{i}.loss"], out[f"lambda_args_{i}.grad"] = run_list(lambda: LambdaLoss(scheme), out["scores_17"], out["grades_17"], **kw)
    np.savez(os.path.join(OUT, "losses_lists.npz"), **out)
    for f in ("losses_pairs.npz", "losses_lists.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
