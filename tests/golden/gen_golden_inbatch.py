#!/usr/bin/env python
"""Generates tests/golden/inbatch_cases.npz by driving the REAL reference loss classes (matchmaker/losses/*.py) on CPU fp32
tensors through the selection of matchmaker/train.py:434-472, restated here with torch operators: inputs, in-batch loss, the
three statistics and the autograd gradients with respect to the vectors and the paired scores.  Data only.  Needs the reference
tree (oracle.ref_harness.REFERENCE_ROOT), so it runs in the build container only; the tests read the file.

    python tests/golden/gen_golden_inbatch.py

Per case c in CASES: <c>.sp [B], .Q, .Dp, .Dn [B, E], .Tp, .Tn [B, B] (teacher cases), .loss, .accuracy, .score_diff,
.teacher_accuracy (pair kinds under a teacher), .g_sp, .g_Q, .g_Dp, .g_Dn.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
# name: (loss kind of tests/losses_reference.py, family, teacher, B, E)
CASES = {"margin_mse_8x16": ("margin_mse", "pair", True, 8, 16), "margin_mse_3x8": ("margin_mse", "pair", True, 3, 8),
         "ranknet_7x12": ("ranknet", "pair", False, 7, 12), "ranknet_teacher_5x8": ("ranknet_teacher", "pair", True, 5, 8),
         "kldiv_6x16": ("kldiv", "list", True, 6, 16), "listnet_4x8": ("listnet", "list", True, 4, 8),
         "lambda_ndcg2_teacher_8x16": ("lambda_ndcg2_teacher", "list", True, 8, 16)}


def inbatch(fn, family, sp, Q, Dp, Dn, Tp, Tn):
    """the block of train.py:434-472 around a loss object: (loss, accuracy, score_diff, teacher accuracy or None)"""
    B = Q.shape[0]
    off = ~torch.eye(B, dtype=torch.bool)
    Sp, Sn = torch.mm(Q, Dp.t()), torch.mm(Q, Dn.t())
    pos = sp.unsqueeze(-1).expand(-1, B - 1).reshape(-1)
    tacc = None
    if Tp is not None and family == "list":
        loss = fn(torch.cat([Sp, Sn], 1), torch.cat([Tp, Tn], 1))
    elif Tp is not None:
        a = Tp[~off].unsqueeze(-1).expand(-1, B - 1).reshape(-1)
        loss = (fn(pos, Sp[off], a, Tp[off]) + fn(pos, Sn[off], a, Tn[off])) * 0.5
        tacc = ((a > Tp[off]).float().mean() + (a > Tn[off]).float().mean()) * 0.5
    else:
        one = torch.ones(pos.shape[0])
        loss = (fn(pos, Sp[off], one) + fn(pos, Sn[off], one)) * 0.5
    acc = ((pos > Sp[off]).float().mean() + (pos > Sn[off]).float().mean()) * 0.5
    diff = ((pos - Sp[off]).mean() + (pos - Sn[off]).mean()) * 0.5
    return loss, acc, diff, tacc


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from gen_golden_losses import reference_classes
    ref = reference_classes()
    rng = np.random.default_rng(24)
    f = np.float32
    out = {}
    for name, (kind, family, teacher, B, E) in CASES.items():
        d = {"sp": f(2 * rng.standard_normal(B)), "Q": f(rng.standard_normal((B, E)) / E ** 0.25),
             "Dp": f(rng.standard_normal((B, E)) / E ** 0.25), "Dn": f(rng.standard_normal((B, E)) / E ** 0.25)}
        if teacher:
            d["Tp"], d["Tn"] = f(3 * rng.standard_normal((B, B))), f(3 * rng.standard_normal((B, B)))
        leaves = {k: torch.from_numpy(d[k]).requires_grad_() for k in ("sp", "Q", "Dp", "Dn")}
        T = [torch.from_numpy(d[k]) if teacher else None for k in ("Tp", "Tn")]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss, acc, diff, tacc = inbatch(ref[kind](), family, leaves["sp"], leaves["Q"], leaves["Dp"], leaves["Dn"], *T)
        loss.backward()
        d.update(loss=loss.detach().numpy(), accuracy=acc.detach().numpy(), score_diff=diff.detach().numpy())
        if tacc is not None:
            d["teacher_accuracy"] = tacc.numpy()
        for k, t in leaves.items():
            d["g_" + k] = t.grad.numpy() if t.grad is not None else np.zeros_like(d[k])
        out.update({f"{name}.{k}": v for k, v in d.items()})
    path = os.path.join(OUT, "inbatch_cases.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
