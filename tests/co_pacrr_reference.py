"""TEST INFRASTRUCTURE — CO-PACRR's per-query block (matchmaker/models/co_pacrr.py:90-158) restated in differentiable torch
ops, evaluated in fp64 by the tests.  Pinned on the REAL class through tests/golden/co_pacrr_*.npz (gen_golden_co_pacrr.py)
and, where the reference tree exists, on live instances (tests/test_co_pacrr_cpu.py).

Tie policy, the native kernel's and PACRR's: descending, lower column first, lowest channel.  In CO-PACRR a
tie also decides WHICH context value is gathered, so the restatement returns the selected columns for the tests' tie
accounting."""
import torch
import torch.nn.functional as F

from tests import pacrr_reference as P

cosine = P.cosine


def views(U):
    """co_pacrr.py:73-74"""
    return [int(U * x) for x in [0.25, 0.5, 0.75, 1]]


def context(q, d):
    """[B, D] ctx[j] = cosine(mean_i q_i, (1/6) sum_{t = j .. j+5} d_t), rows past D as zeros (:98-101, :65-68)."""
    qc = q.mean(dim=1, keepdim=True)
    dc = F.avg_pool1d(F.pad(d.transpose(1, 2), (0, 5)), kernel_size=6, stride=1).transpose(1, 2)
    return cosine(qc, dc)[:, 0]


def _paths(cos, weights, biases):
    """[path 0 = cos, path n = channel max of the padded n x n conv] as in pacrr_reference.per_query_results."""
    B, Q, D = cos.shape
    out = [cos]
    for w, b in zip(weights, biases):
        n = w.shape[-1]
        cols_ = F.unfold(F.pad(cos[:, None], (0, n - 1, 0, n - 1)), n)
        cr = (torch.matmul(w.reshape(w.shape[0], -1), cols_) + b[:, None]).view(B, -1, Q, D)
        ch = cr.detach().argmax(dim=1, keepdim=True)
        out.append(torch.gather(cr, 1, ch)[:, 0])
    return out


def per_query_results(q, d, weights, biases, k, U, pairs_per_query=1, return_columns=False):
    """[B, Q, 8 k N]: per path 0, 2, .., N the top-k of views 0..3 (4k values), then ctx at those 4k columns.
    q [n_queries, Q, E], d [B, D, E]; weights[i] [C, 1, n, n], biases[i] [C] for n = i + 2; U the unified document length.
    return_columns: also the int64 columns [B, Q, N, 4k]."""
    if pairs_per_query > 1:
        q = q.repeat_interleave(pairs_per_query, dim=0)[:d.shape[0]]
    ctx = context(q, d)
    B, Q = q.shape[0], q.shape[1]
    blocks, cols = [], []
    for path in _paths(cosine(q, d), weights, biases):
        vals, cs = [], []
        for v in views(U):
            val, c = P.topk_stable(path[:, :, 0:v], k)
            vals.append(val)
            cs.append(c)
        c = torch.cat(cs, dim=-1)
        sel = torch.gather(ctx[:, None, :].expand(B, Q, ctx.shape[1]), -1, c)
        blocks.append(torch.cat(vals + [sel], dim=-1))
        cols.append(c)
    out = torch.cat(blocks, dim=-1)
    if return_columns:
        return out, torch.stack(cols, dim=2)
    return out


score = P.score


def paths(q, d, weights, biases, pairs_per_query=1):
    """The N path matrices [B, Q, D] (cosine, then the conv channel maxima), detached."""
    if pairs_per_query > 1:
        q = q.repeat_interleave(pairs_per_query, dim=0)[:d.shape[0]]
    return [p.detach() for p in _paths(cosine(q, d), weights, biases)]


def compare_context_slots(got, ref, path_mats, k, U, atol, tie_tol=1e-6, return_pairs=False):
    """Compares the context slots of per_query_results `got` against `ref` [B, Q, 8 k N] under the tie rules of DESIGN.md
    §3.8.  path_mats: the fp64 path matrices (paths()), which decide the ties.  Per value slot of view i:
      * its fp64 value is separated from every other column of the view by more than tie_tol: the context must match;
      * it belongs to a tied group that lies wholly inside the top-k: the group's contexts must match as a multiset;
      * its tied group straddles the k-th place: which contexts land there is implementation-defined — excluded.
    Returns the number of excluded slots, and with return_pairs the [B] mask of the pairs that hold any tied group: there the
    order of the tied slots, and with it which context (and which gradient route) lands in which slot, is the
    implementation's.  The value slots are not compared here."""
    ref = ref.detach().double()
    got = got.detach().double().to(ref.device)
    B, Q, _ = ref.shape
    N = len(path_mats)
    excluded = 0
    pairs = torch.zeros(B, dtype=torch.bool, device=ref.device)
    for p, pm in enumerate(path_mats):
        pm = pm.double().to(ref.device)
        D = pm.shape[-1]
        blk = slice(p * 8 * k, (p + 1) * 8 * k)
        rb, gb = ref[..., blk], got[..., blk]
        for i, v in enumerate(views(U)):
            vals = pm[:, :, :min(v, D)]
            sel = rb[..., i * k:(i + 1) * k]                                     # [B, Q, k] values
            n_view = ((vals[..., None, :] - sel[..., :, None]).abs() <= tie_tol).sum(-1)   # [B, Q, k]
            n_sel = ((sel[..., None, :] - sel[..., :, None]).abs() <= tie_tol).sum(-1)
            rc, gc = rb[..., 4 * k + i * k:4 * k + (i + 1) * k], gb[..., 4 * k + i * k:4 * k + (i + 1) * k]
            unique = n_view == 1
            err = float(torch.cat([(rc - gc).abs()[unique], rc.new_zeros(1)]).max())
            assert err <= atol, ("context slots", p, i, err)
            inside = (n_view > 1) & (n_view == n_sel)
            excluded += int((n_view > n_sel).sum())
            pairs |= (n_view > 1).flatten(1).any(1)
            for b, r in torch.nonzero(inside.any(-1)).tolist():
                s = sel[b, r]
                done = torch.zeros(k, dtype=torch.bool, device=ref.device)
                for j in range(k):
                    if not inside[b, r, j] or done[j]:
                        continue
                    grp = (s - s[j]).abs() <= tie_tol
                    done |= grp
                    a, c = torch.sort(rc[b, r][grp]).values, torch.sort(gc[b, r][grp]).values
                    assert float((a - c).abs().max()) <= atol, (p, i, b, r)
    assert N == ref.shape[-1] // (8 * k)
    return (excluded, pairs) if return_pairs else excluded
