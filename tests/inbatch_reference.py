"""Float64 numpy restatement of the in-batch negatives of matchmaker/train.py:434-472 (a helper like tests/losses_reference.py,
not a test module): the selection of the off-diagonal pairs, the loss through tests/losses_reference.py, the three statistics
and every gradient.  Inputs are widened exactly to float64; nothing is rounded on the way.

    Sp = Q Dp^T, Sn = Q Dn^T;  M = B (B - 1);  "off" = every (i, j) with i != j, row-major
    pair kinds   loss = (mean_off l(sp_i, Sp_ij; a_i, b_ij) + mean_off l(sp_i, Sn_ij; a_i, b'_ij)) / 2 with a_i = Tp_ii, b = Tp_ij,
                 b' = Tn_ij under a teacher, else the label 1
    list kinds   the list loss of cat([Sp, Sn], 1) against cat([Tp, Tn], 1), the diagonal included, sp unused
    accuracy = (mean_off [sp_i > Sp_ij] + mean_off [sp_i > Sn_ij]) / 2, score_diff alike with sp_i - S_ij, teacher accuracy alike
    with Tp_ii > T_ij (pair kinds under a teacher only)
"""
import numpy as np

from tests import losses_reference as R

ONE_LABEL = ("ranknet", "margin")


def f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def off_mask(B):
    return ~np.eye(B, dtype=bool)


def counts(sp, Sp, Sn, Tp=None, Tn=None):
    """(greater, M2, teacher greater or None): the integer numerators of accuracy and teacher accuracy and their denominator 2 M"""
    sp, Sp, Sn = f64(sp), f64(Sp), f64(Sn)
    off = off_mask(Sp.shape[0])
    n = int((sp[:, None] > Sp)[off].sum() + (sp[:, None] > Sn)[off].sum())
    t = None
    if Tp is not None:
        d = np.diagonal(f64(Tp))[:, None]
        t = int((d > f64(Tp))[off].sum() + (d > f64(Tn))[off].sum())
    return n, 2 * int(off.sum()), t


def from_scores(family, kind, sp, Sp, Sn, Tp=None, Tn=None):
    """dict(loss, accuracy, score_diff, teacher_accuracy (None where undefined), g_sp [B], g_Sp, g_Sn [B, B]) in float64"""
    sp, Sp, Sn, Tp, Tn = f64(sp), f64(Sp), f64(Sn), f64(Tp), f64(Tn)
    B = Sp.shape[0]
    off = off_mask(B)
    M = B * (B - 1)
    out = {"g_sp": np.zeros(B), "g_Sp": np.zeros((B, B)), "g_Sn": np.zeros((B, B)), "teacher_accuracy": None}
    n, M2, t = counts(sp, Sp, Sn, Tp, Tn)
    nan = float("nan")
    out["accuracy"] = n / M2 if M2 else nan
    out["score_diff"] = ((sp[:, None] - Sp)[off].sum() + (sp[:, None] - Sn)[off].sum()) / M2 if M2 else nan
    if family == "list":
        loss, _, grad = R.lists(kind, np.concatenate([Sp, Sn], 1), np.concatenate([Tp, Tn], 1))
        out["loss"], out["g_Sp"], out["g_Sn"] = float(loss), f64(grad)[:, :B], f64(grad)[:, B:]
        return out
    if Tp is not None:
        out["teacher_accuracy"] = t / M2 if M2 else nan
    if M == 0:
        out["loss"] = nan
        return out
    pos = np.repeat(sp, B - 1)
    a = np.repeat(np.diagonal(Tp), B - 1) if Tp is not None else np.ones(M)
    loss = 0.0
    for S, T, key in ((Sp, Tp, "g_Sp"), (Sn, Tn, "g_Sn")):
        labels = (a,) if kind in ONE_LABEL else (a, T[off])
        l, gpos, gneg = R.pair(kind, pos, S[off], *labels)
        loss += 0.5 * float(l)
        out["g_sp"] += 0.5 * f64(gpos).reshape(B, B - 1).sum(1)
        out[key][off] = 0.5 * f64(gneg)
    out["loss"] = loss
    return out


def from_vectors(family, kind, sp, Q, Dp, Dn, Tp=None, Tn=None):
    """from_scores on Sp = Q Dp^T, Sn = Q Dn^T (the query of the positive pair for both), plus Sp, Sn and g_Q, g_Dp, g_Dn [B, E]"""
    Q, Dp, Dn = f64(Q), f64(Dp), f64(Dn)
    Sp, Sn = Q @ Dp.T, Q @ Dn.T
    out = from_scores(family, kind, sp, Sp, Sn, Tp, Tn)
    out.update(Sp=Sp, Sn=Sn, g_Q=out["g_Sp"] @ Dp + out["g_Sn"] @ Dn, g_Dp=out["g_Sp"].T @ Q, g_Dn=out["g_Sn"].T @ Q)
    return out


def dot_bound(Q, D):
    """[B, B]: the fp32 dot bound E 2^-24 sum_k |q_k d_k| of every (query, document) pair"""
    Q, D = np.abs(f64(Q)), np.abs(f64(D))
    return Q.shape[1] * 2.0 ** -24 * (Q @ D.T)
