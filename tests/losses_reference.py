"""float64 numpy restatement of every kind of mm_pair_loss_fwd / mm_list_loss_fwd with ANALYTIC gradients (a helper like
tests/abi.py, not a test module): the yardstick of tests/test_losses_cpu.py and tests/test_losses_gpu.py.  It follows the
formulas of include/mm_native.h, not the kernel: sorted positions and a pair loop for the Lambda kinds, a plain softmax
Jacobian for ListNet / KLDiv.  Inputs are taken as they are (fp32 or 16-bit values widened) and computed in float64."""
import numpy as np

EPS = np.float64(np.float32(1e-6))      # the reference clamps fp32 tensors at the Python float 1e-6: the fp32 value
LN2 = np.log(2.0)

PAIR_KINDS = ("ranknet", "margin", "margin_mse", "mse_pointwise", "kldiv_pointwise", "ranknet_teacher", "mse_ranknet")
LIST_KINDS = ("listnet", "kldiv", "smooth_mrr", "lambda_ndcg2", "lambda_ndcg2_teacher")
# LambdaLoss arguments the kernel does not implement (weighing scheme, forward keywords): they run the eager formula, and
# tests/golden/losses_lists.npz holds the reference's result of each on scores_17 / grades_17 as lambda_args_<i>.loss / .grad
LAMBDA_ARG_CASES = (
    (None, {}), ("ndcgLoss1_scheme", {}), ("lamdbaRank_scheme", {}), ("ndcgLoss2PP_scheme", {"mu": 3.0}), ("rankNet_scheme", {}),
    ("rankNetWeightedByGTDiff_scheme", {}), ("rankNetWeightedByGTDiffPowed_scheme", {}), ("ndcgLoss2_scheme", {"k": 5}),
    ("ndcgLoss2_scheme", {"sigma": 2.0}), ("ndcgLoss2_scheme", {"reduction": "mean"}), ("ndcgLoss2_scheme", {"reduction_log": "natural"}))


def f64(x):
    return np.asarray(x, dtype=np.float64)


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def xlogx(t):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(t == 0, 0.0, t * np.log(t))


def pair(kind, pos, neg, a, b=None):
    """(loss, grad_pos, grad_neg) in float64; the mean over n, gradients with the 1 / n."""
    pos, neg, a = f64(pos).ravel(), f64(neg).ravel(), f64(a).ravel()
    b = f64(b).ravel() if b is not None else None
    n, x = pos.size, pos - neg
    if kind == "ranknet":
        t, dx = softplus(x) - x * a, sigmoid(x) - a
        gp, gn = dx, -dx
    elif kind == "margin":
        h = 1.0 - a * x
        t, dx = np.maximum(h, 0.0), np.where(h >= 0, -a, 0.0)
        gp, gn = dx, -dx
    elif kind == "margin_mse":
        d = x - (a - b)
        t, gp, gn = d * d, 2 * d, -2 * d
    elif kind == "mse_pointwise":
        t, gp, gn = ((pos - a) ** 2 + (neg - b) ** 2) / 2, pos - a, neg - b
    elif kind == "kldiv_pointwise":
        t, gp, gn = (xlogx(a) - a * pos + xlogx(b) - b * neg) / 2, -a / 2, -b / 2
    elif kind == "ranknet_teacher":
        t, dx = (a - b) * (softplus(x) - x), (a - b) * (sigmoid(x) - 1.0)
        gp, gn = dx, -dx
    elif kind == "mse_ranknet":
        dx = sigmoid(x) - 1.0
        t, gp, gn = ((pos - a) ** 2 + (neg - b) ** 2) / 2 + softplus(x) - x, (pos - a) + dx, (neg - b) - dx
    else:
        raise KeyError(kind)
    return (t.sum() / n if n else np.float64("nan")), gp / max(n, 1), gn / max(n, 1)


def softmax(v):
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def stable_desc_order(s):
    """indices of one list, higher score first, equal scores in arrival order, -0 == +0 (mm_segment_rank_fwd's rule)"""
    return np.argsort(-(s + 0.0), kind="stable")


def teacher_labels(labels32):
    """LambdaLossTeacher's labels: softmax in fp32 (exp, the sum and the division as the header states them), + 2 where > 0.001.
    Returned as float64 of the fp32 values, with the softmax itself for the input-condition checks."""
    y = np.asarray(labels32, dtype=np.float32)
    e = np.exp((y - y.max(axis=-1, keepdims=True)).astype(np.float64))
    T = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    return f64(np.where(T > np.float32(0.001), T + np.float32(2.0), T)), T


def lambda_pairs(s, y):
    """The counted pairs of ONE list (lambda_ndcg2, labels already final): arrays (i, j, w, x) over sorted positions, and the
    order.  y == -1 is padded."""
    s, y = f64(s).copy(), f64(y).copy()
    pad = y == -1
    s[pad], y[pad] = -np.inf, -np.inf
    order = stable_desc_order(s)
    ss, t = s[order], y[order]
    L = s.size
    D = np.log2(2.0 + np.arange(L))
    gains_sorted = 2.0 ** np.maximum(np.sort(y)[::-1], 0.0) - 1.0
    max_dcg = max((gains_sorted / D).sum(), EPS)
    G = (2.0 ** np.maximum(t, 0.0) - 1.0) / max_dcg
    ii, jj = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(t)[:, None] & np.isfinite(t)[None, :] & (t[:, None] > t[None, :])
    ii, jj = ii[keep], jj[keep]
    gap = np.abs(ii - jj)
    w = np.abs(1.0 / D[gap - 1] - 1.0 / D[gap]) * np.abs(G[ii] - G[jj])
    x = np.clip(ss[ii] - ss[jj], -1e4, 1e4)
    return ii, jj, w, x, order


def _lambda_one(s, y):
    ii, jj, w, x, order = lambda_pairs(s, y)
    p = sigmoid(x)
    pw = np.maximum(p, EPS) ** w
    loss = -np.log2(np.maximum(pw, EPS)).sum()
    gx = np.where((p >= EPS) & (pw >= EPS), -w * (1.0 - p) / LN2, 0.0)
    g_sorted = np.zeros(len(s))
    np.add.at(g_sorted, ii, gx)
    np.add.at(g_sorted, jj, -gx)
    g = np.zeros(len(s))
    g[order] = g_sorted
    return loss, g


def smooth_mrr_rr(scores):
    s = f64(scores)
    return 1.0 / (0.5 + sigmoid(s[:, None, :] - s[:, :, None]).sum(-1))      # 1 / rank_i, rank_i = 0.5 + sum_j sg(s_j - s_i)


def lists(kind, scores, labels):
    """(loss, per_list [B], grad [B, L]) in float64."""
    s, y = f64(scores), f64(labels)
    B, L = s.shape
    g = np.zeros_like(s)
    if kind in ("listnet", "kldiv"):
        p, T = softmax(s), softmax(y)
        if kind == "listnet":
            per = -(T * np.log(p + EPS)).sum(-1)
            q = T * p / (p + EPS)
        else:
            per = (xlogx(T) - T * p).sum(-1)
            q = T * p
        g = -(q - p * q.sum(-1, keepdims=True)) / B
        return per.sum() / B, per, g
    if kind == "smooth_mrr":
        rr = np.where(y > 0, smooth_mrr_rr(s), 0.0)
        b = rr.argmax(-1)                                           # numpy: the first of tied maxima = the lowest index
        per = 1.0 - rr[np.arange(B), b]
        for r in range(B):
            if rr[r, b[r]] <= 0:
                continue
            sg = sigmoid(s[r] - s[r, b[r]])
            d = sg * (1.0 - sg)
            d[b[r]] = 0.0
            row = d.copy()
            row[b[r]] = -d.sum()
            g[r] = row * rr[r, b[r]] ** 2 / B
        return per.sum() / B, per, g
    if kind == "lambda_ndcg2_teacher":
        y = teacher_labels(labels)[0]
    elif kind != "lambda_ndcg2":
        raise KeyError(kind)
    per = np.zeros(B)
    for r in range(B):
        per[r], g[r] = _lambda_one(s[r], y[r])
    return per.sum(), per, g


# ---- units of the GPU tests' tolerance (the rule itself: check() in tests/test_losses_gpu.py) ----------------------------
def ulp32(x):
    """the fp32 ulp at |x| (of the smallest normal below it)"""
    x = np.maximum(np.abs(f64(x)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def round16(x, dtype):
    """float64 -> the nearest fp16 / bf16 value (as float64), through torch"""
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dtype).to(torch.float64).numpy()


def ulp16(x, dtype):
    import torch
    bits = 8 if dtype == torch.bfloat16 else 11
    emin = -126 if dtype == torch.bfloat16 else -14
    x = np.maximum(np.abs(f64(x)), 2.0 ** emin)
    return 2.0 ** (np.floor(np.log2(x)) - (bits - 1))
