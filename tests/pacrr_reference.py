"""TEST INFRASTRUCTURE — PACRR's per-query k-max block (matchmaker/models/pacrr.py:78-97) restated in differentiable torch ops,
evaluated in fp64 by the tests.  The restatement is pinned on the REAL class through tests/golden/pacrr_*.npz
(gen_golden_pacrr.py) and, where the reference tree exists, on live instances (tests/test_pacrr_cpu.py).

Tie policy, the native kernel's: top-k values are sorted descending and equal values keep the lower document
column first (a stable sort); the channel max picks the lowest channel among equal ones (MaxPool3d's first maximum)."""
import torch
import torch.nn.functional as F


def cosine(q, d):
    """allennlp cosine: x / (|x|_2 + 1e-13), then bmm (pacrr.py:78)."""
    qn = q / (q.norm(p=2, dim=-1, keepdim=True) + 1e-13)
    dn = d / (d.norm(p=2, dim=-1, keepdim=True) + 1e-13)
    return torch.bmm(qn, dn.transpose(-1, -2))


def topk_stable(x, k):
    """(values, columns) of the k largest entries of every row of x [..., D], descending, lower column first on ties."""
    order = torch.sort(x.detach(), dim=-1, descending=True, stable=True).indices[..., :k]
    return torch.gather(x, -1, order), order


def per_query_results(q, d, weights, biases, k, pairs_per_query=1, return_positions=False):
    """[B, Q, k N]: path 0 (the cosine), then widths n = 2 .. N (pad right / bottom by n - 1, conv, max over channels).
    q [n_queries, Q, E], d [B, D, E]; weights[i] [C, 1, n, n], biases[i] [C] for n = i + 2.
    return_positions: also the int64 columns [B, Q, k N] and the winning channels (0 on path 0)."""
    if pairs_per_query > 1:
        q = q.repeat_interleave(pairs_per_query, dim=0)[:d.shape[0]]
    cos = cosine(q, d)
    vals, cols, chans = [], [], []
    v, c = topk_stable(cos, k)
    vals.append(v)
    cols.append(c)
    chans.append(torch.zeros_like(c))
    B, Q, D = cos.shape
    for w, b in zip(weights, biases):
        n = w.shape[-1]
        # Conv2d as im2col + matmul (any dtype on any device): [C, n^2] x [n^2, Q D] + bias
        cols_ = F.unfold(F.pad(cos[:, None], (0, n - 1, 0, n - 1)), n)            # [B, n^2, Q D]
        cr = (torch.matmul(w.reshape(w.shape[0], -1), cols_) + b[:, None]).view(B, -1, Q, D)   # [B, C, Q, D]
        ch = cr.detach().argmax(dim=1, keepdim=True)                              # first maximum
        m = torch.gather(cr, 1, ch)[:, 0]
        v, c = topk_stable(m, k)
        vals.append(v)
        cols.append(c)
        chans.append(torch.gather(ch[:, 0], -1, c))
    out = torch.cat(vals, dim=-1)
    if return_positions:
        return out, torch.cat(cols, dim=-1), torch.cat(chans, dim=-1)
    return out


def score(pqr, dense_w, dense_b, dense2_w, dense2_b, dense3_w):
    """pacrr.py:101-112 on per_query_results [B, Q, k N]."""
    x = pqr.reshape(pqr.shape[0], -1)
    x = F.relu(F.linear(x, dense_w, dense_b))
    x = F.relu(F.linear(x, dense2_w, dense2_b))
    return F.linear(x, dense3_w).squeeze(1)
