"""numpy float64 restatement of the backward of the all-pairs MaxSim (matchmaker/models/colbert.py:154-162, as
oracle/torch_port.maxsim_inbatch restates the forward): the arg-max table with the FIRST position on ties, both gradients,
and per gradient element the sum of absolute terms and the number of terms (what an error bound of a float32 sum needs).

    j*(i, j, t) = first arg-max over p of ( keep[m, p] ? <q[i, t], d[j, p]> : -1000 ),  m = j (m = i: bug-compatible, Bq == Bd)
    no gradient: padded query token, or the arg-max is a masked position
    grad_q[i, t] = sum_j grad_out[i, j] d[j, j*]            grad_d[j, p] = sum_i sum_{t: j* = p} grad_out[i, j] q[i, t]
"""
import numpy as np


def similarities(q, d, d_mask, bug_compatible=False):
    """(masked similarities [Bq, Bd, Q, D] float64, keep [Bq or 1, Bd or 1, 1, D] as broadcast against them)."""
    q = np.asarray(q, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    Bq, Bd = q.shape[0], d.shape[0]
    keep = np.asarray(d_mask) != 0
    if bug_compatible:
        if Bq != Bd:
            raise ValueError("bug-compatible masking needs Bq == Bd")
        keep = keep[:, None, None, :]
    else:
        keep = keep[None, :, None, :]
    s = np.einsum("ite,jpe->ijtp", q, d)
    return np.where(keep, s, -1000.0), np.broadcast_to(keep, s.shape)


def argmax_table(q, q_mask, d, d_mask, bug_compatible=False):
    """int64 [Bq, Bd, Q]: first arg-max document position, -1 where no gradient flows."""
    s, keep = similarities(q, d, d_mask, bug_compatible)
    js = s.argmax(-1)                                          # numpy: first occurrence of the maximum
    real = np.take_along_axis(keep, js[..., None], -1)[..., 0]
    qm = (np.asarray(q_mask) != 0)[:, None, :]
    return np.where(real & qm, js, -1)


def gaps(q, q_mask, d, d_mask, bug_compatible=False):
    """(best - second-best masked similarity [Bq, Bd, Q], cells that carry a gradient [Bq, Bd, Q], max |similarity| of real positions)."""
    s, keep = similarities(q, d, d_mask, bug_compatible)
    tab = argmax_table(q, q_mask, d, d_mask, bug_compatible)
    top2 = np.partition(s, -2, axis=-1)[..., -2:]
    return top2[..., 1] - top2[..., 0], tab >= 0, float(np.abs(np.where(keep, s, 0.0)).max())


def min_gap(q, q_mask, d, d_mask, bug_compatible=False):
    """(smallest gap over the cells that carry a gradient, max |similarity| of real positions)."""
    gap, decided, mx = gaps(q, q_mask, d, d_mask, bug_compatible)
    gap = gap[decided]
    return (float(gap.min()) if gap.size else float("inf")), mx


def gradients(q, q_mask, d, d_mask, grad_out, bug_compatible=False):
    """dict: gq [Bq,Q,E], gd [Bd,D,E] float64; aq, ad = sum of |grad_out * x| per element; nq [Bq,Q,1], nd [Bd,D,1] = terms per element."""
    q = np.asarray(q, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    go = np.asarray(grad_out, dtype=np.float64)
    Bq, Q, E = q.shape
    Bd, D, _ = d.shape
    tab = argmax_table(q, q_mask, d, d_mask, bug_compatible)
    gq, aq, nq = np.zeros((Bq, Q, E)), np.zeros((Bq, Q, E)), np.zeros((Bq, Q, 1))
    gd, ad, nd = np.zeros((Bd, D, E)), np.zeros((Bd, D, E)), np.zeros((Bd, D, 1))
    for i in range(Bq):
        for j in range(Bd):                                   # ascending j, then ascending t: the native order as well
            t = np.nonzero(tab[i, j] >= 0)[0]
            if t.size == 0:
                continue
            p = tab[i, j, t]
            g = go[i, j]
            gq[i, t] += g * d[j, p]
            aq[i, t] += np.abs(g * d[j, p])
            nq[i, t] += 1
            np.add.at(gd[j], p, g * q[i, t])
            np.add.at(ad[j], p, np.abs(g * q[i, t]))
            np.add.at(nd[j], p, 1)
    return {"table": tab, "gq": gq, "gd": gd, "aq": aq, "ad": ad, "nq": nq, "nd": nd}


def bound(ref, abs_terms, n_terms, u_out, tiny=0.0):
    """|got - ref64| <= (n + 2) 2^-24 sum|terms| + u_out |ref64| (+ tiny): a float32 sum of n products of float32-exact factors in
    any order (n - 1 additions and n product roundings, each relative 2^-24, to first order n 2^-24 sum|terms|; + 2 for slack of
    the higher-order terms) and one rounding to the output type.  u_out |ref64| holds for normal numbers only: float16 is
    spaced 2^-24 below 2^-14, so where |ref64| < 2^-14 rounding to it adds up to tiny = 2^-25 in absolute terms — without
    that term the correctly rounded float64 gradient itself misses the bound (float32 and bfloat16 underflow near 1e-38: no
    term).  Elements at or above 2^-14 get the plain formula."""
    ref = np.asarray(ref)
    return (n_terms + 2) * 2.0 ** -24 * abs_terms + u_out * np.abs(ref) + np.where(np.abs(ref) < 2.0 ** -14, tiny, 0.0)
