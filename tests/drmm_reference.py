"""TEST INFRASTRUCTURE — DRMM's scoring block (matchmaker/models/drmm.py:66-91) restated in torch ops, evaluated in fp64 by
the tests: allennlp's cosine, torch.histc's bin rule, log1p + FeedForward(tanh, tanh) + masked softmax gate.  Pinned on the
REAL class through tests/golden/drmm_*.npz (gen_golden_drmm.py) and, where the reference tree exists, on live instances
(tests/test_drmm_cpu.py).

Bin decisions are discontinuous, and exact matches (cosine 1 +- a few ulp) are dropped by histc when they round above 1: no
two evaluations agree element for element.  So histograms are compared through DECIDED elements: with c64
the fp64 cosine, an element is undecided when c64 lies within `tol` of one of the bins + 1 edges and is not exactly 0 (a
zero row); bounds() turns that into per-bin lower / upper counts."""
import torch


def cosine(q, d):
    """allennlp cosine: x / (|x|_2 + 1e-13), then bmm (drmm.py:66)."""
    qn = q / (q.norm(p=2, dim=-1, keepdim=True) + 1e-13)
    dn = d / (d.norm(p=2, dim=-1, keepdim=True) + 1e-13)
    return torch.bmm(qn, dn.transpose(-1, -2))


def expand_queries(q, B, pairs_per_query=1):
    return q.repeat_interleave(pairs_per_query, dim=0)[:B] if pairs_per_query > 1 else q


def histc_rows(cos, bins):
    """torch.histc(row, bins, min=-1, max=1) for every row of cos [..., D] at once, in cos's dtype: an element below -1 or
    above 1 is dropped, otherwise its bin is min(int((x + 1) / 2 * bins), bins - 1); x == 1 lands in the last bin."""
    inr = (cos >= -1) & (cos <= 1)
    b = ((cos + 1) / 2 * bins).to(torch.int64).clamp(0, bins - 1)
    out = torch.zeros(cos.shape[:-1] + (bins,), dtype=cos.dtype)
    return out.scatter_add_(-1, b, inr.to(cos.dtype))


def histogram(q, d, bins, pairs_per_query=1):
    return histc_rows(cosine(expand_queries(q, d.shape[0], pairs_per_query), d), bins)


def feed_forward(x, w0, b0, w1, b1):
    """allennlp FeedForward(num_layers=2, activations tanh, tanh), dropout 0."""
    return torch.tanh(torch.tanh(x @ w0.T + b0) @ w1.T + b1)


def masked_softmax(x, mask):
    """drmm.py:97-120."""
    x_masked = x * mask + (1 - 1 / mask)
    x_exp = (x - x_masked.max(1)[0].unsqueeze(-1)).exp() * mask
    return x_exp / x_exp.sum(1).unsqueeze(-1)


def gate(q, q_mask, p):
    """[nq, Q]: the masked softmax of query_gate (drmm.py:82-83); p = the state_dict as fp64 tensors."""
    raw = feed_forward(q, p["query_gate._linear_layers.0.weight"], p["query_gate._linear_layers.0.bias"],
                       p["query_gate._linear_layers.1.weight"], p["query_gate._linear_layers.1.bias"])
    return masked_softmax(raw.squeeze(-1), q_mask)


def head(hist, gates, p):
    """[B, 1] = sum_q classified * gate (drmm.py:77, :88); gates [B, Q]."""
    c = feed_forward(torch.log1p(hist), p["matching_classifier._linear_layers.0.weight"],
                     p["matching_classifier._linear_layers.0.bias"], p["matching_classifier._linear_layers.1.weight"],
                     p["matching_classifier._linear_layers.1.bias"])
    return torch.sum(c * gates.unsqueeze(-1), dim=1)


def score(q, d, q_mask, p, bins, pairs_per_query=1):
    g = expand_queries(gate(q, q_mask, p), d.shape[0], pairs_per_query)
    return head(histogram(q, d, bins, pairs_per_query), g, p)


def params64(g):
    return {k[len("param."):]: torch.tensor(v, dtype=torch.float64) for k, v in g.items() if k.startswith("param.")}


def measured_tol(q, d, pairs_per_query=1):
    """4 x max |c32 - c64| of the fp32 torch restatement on the CPU (never the kernel's output); the factor 4 covers the
    kernel's different summation order."""
    q, d = q.detach().cpu(), d.detach().cpu()
    qq = expand_queries(q, d.shape[0], pairs_per_query)
    c32 = cosine(qq.float(), d.float()).double()
    c64 = cosine(qq.double(), d.double())
    return 4.0 * float((c32 - c64).abs().max())


def bounds(q, d, bins, tol, pairs_per_query=1, q_rows=None):
    """Per (pair, query row, bin) lower / upper counts from the fp64 cosine c64 and the row-total bounds.

    decided: c64 further than tol from every edge, or c64 == 0 exactly; lower counts the decided elements of a bin, upper
    adds the undecided elements at the bin's two edges (at -1 / +1: the edge bin, or dropped).  Returns a dict with lower,
    upper [B, Q, bins], total_lo, total_hi [B, Q], undecided (count over the query rows `q_rows` [B, Q] bool, default all)
    and share = undecided / elements of those rows."""
    q, d = q.detach().cpu().double(), d.detach().cpu().double()
    c = cosine(expand_queries(q, d.shape[0], pairs_per_query), d)
    B, Q, D = c.shape
    edges = -1.0 + 2.0 * torch.arange(bins + 1, dtype=torch.float64) / bins
    dist = (c.unsqueeze(-1) - edges).abs()                       # [B, Q, D, bins + 1]
    near = dist.argmin(-1)
    und = (dist.min(-1)[0] < tol) & (c != 0)
    dec = ~und
    inr = (c >= -1) & (c <= 1)
    b = ((c + 1) / 2 * bins).to(torch.int64).clamp(0, bins - 1)
    lower = torch.zeros(B, Q, bins, dtype=torch.float64).scatter_add_(-1, b, (dec & inr).double())
    upper = lower.clone()
    left = (near - 1).clamp(0, bins - 1)                         # the bin below the edge (edge 0: none -> masked out)
    right = near.clamp(0, bins - 1)                              # the bin above the edge (edge `bins`: none)
    upper.scatter_add_(-1, left, (und & (near >= 1)).double())
    upper.scatter_add_(-1, right, (und & (near <= bins - 1)).double())
    total_lo = (dec & inr).double().sum(-1)
    total_hi = total_lo + und.double().sum(-1)
    rows = torch.ones(B, Q, dtype=torch.bool) if q_rows is None else q_rows
    n_und = int((und & rows.unsqueeze(-1)).sum())
    return {"lower": lower, "upper": upper, "total_lo": total_lo, "total_hi": total_hi, "undecided": n_und,
            "share": n_und / max(1, int(rows.sum()) * D), "c64": c}


def check_hist(hist, bd, tol, label=""):
    """Asserts lower <= hist <= upper per bin and the row-total rule."""
    h = hist.detach().cpu().double()
    msg = f"{label}: tol = {tol:.3e}, undecided = {bd['undecided']} (share {bd['share']:.3e})"
    assert (h >= bd["lower"]).all() and (h <= bd["upper"]).all(), msg + ": a bin count outside its decided bounds"
    tot = h.sum(-1)
    assert (tot >= bd["total_lo"]).all() and (tot <= bd["total_hi"]).all(), msg + ": a row total outside its bounds"
