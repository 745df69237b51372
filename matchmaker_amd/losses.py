"""Training losses with a native route: drop-ins for matchmaker/losses/*.py (same class names, constructors and forward
signatures) over two fused operators of libmm_native.so (csrc/losses.hip):

    pair_loss(pos, neg, a, b, kind)  -> (loss, grad_pos, grad_neg)      mm_pair_loss_fwd
    list_loss(scores, labels, kind)  -> (loss, per_list, grad)          mm_list_loss_fwd

Each call returns the reduced loss AND its gradient with respect to the scores, so autograd's backward is one multiply by
grad_output.  Every class also holds its own eager torch formula, which runs for CPU tensors, labels that require grad,
shapes that do not match, lists longer than MAX_LIST and, for LambdaLoss, every argument the kernel does not implement
(other weighing schemes, k, sigma != 1, reduction="mean", the natural logarithm); `native = False` on a class or an instance
selects it everywhere.  The default of each class follows the measurement rule of DESIGN 3.22: True where the native route
was faster than the eager one in every measured leg by more than the spread of two rounds (all but RankNetLoss and
MSMarginLoss).

A call that takes the native route and fails raises: nothing falls back after the decision.

The torch <-> ABI wrappers live here, not in ops.py; the module has its own `torch`, `_workspace` and `clear_workspaces`
names and allocates its outputs with `torch.empty`, so tests/poison.py can be pointed at it.

Out of scope (they run the reference's own code): MSETeacherPointwisePassages, MarginMSE_InterPassageLoss, the QA loss,
merge_loss, and the `mrr` statistic of train.py:369-374.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from ._lib import NativeError
from .ops import _DT, _call, _dev_check, _workspace, clear_workspaces  # noqa: F401  (re-exported: tests/poison.py patches them here)

MAX_LIST = _lib.LOSS_MAX_LIST
PAIR_KINDS = {"ranknet": _lib.PAIR_RANKNET, "margin": _lib.PAIR_MARGIN, "margin_mse": _lib.PAIR_MARGIN_MSE,
              "mse_pointwise": _lib.PAIR_MSE_POINTWISE, "kldiv_pointwise": _lib.PAIR_KLDIV_POINTWISE,
              "ranknet_teacher": _lib.PAIR_RANKNET_TEACHER, "mse_ranknet": _lib.PAIR_MSE_RANKNET}
LIST_KINDS = {"listnet": _lib.LIST_LISTNET, "kldiv": _lib.LIST_KLDIV, "smooth_mrr": _lib.LIST_SMOOTH_MRR,
              "lambda_ndcg2": _lib.LIST_LAMBDA_NDCG2, "lambda_ndcg2_teacher": _lib.LIST_LAMBDA_NDCG2_TEACHER}
_ONE_LABEL = (_lib.PAIR_RANKNET, _lib.PAIR_MARGIN)
_SUM_KINDS = (_lib.LIST_LAMBDA_NDCG2, _lib.LIST_LAMBDA_NDCG2_TEACHER)      # reduction="sum": no division by B


def _kind(table, kind, op):
    k = table.get(kind, kind) if isinstance(kind, str) else kind
    if k not in table.values():
        raise NativeError(f"{op}: unknown kind {kind!r} (one of {sorted(table)})", _lib.MM_EINVAL)
    return k


def _label32(t, shape, op, name):
    if t.shape != shape:
        raise NativeError(f"{op}: {name} has shape {tuple(t.shape)}, the scores {tuple(shape)}")
    return t.detach().to(torch.float32).contiguous()


# ---- torch <-> ABI ---------------------------------------------------------------------------------------------------------
def pair_loss(pos, neg, a, b, kind):
    """(loss [] float32, grad_pos, grad_neg like pos / neg) of a pairwise / pointwise loss (native mm_pair_loss_fwd).

    pos, neg: float32 / float16 / bfloat16 tensors of one shape and dtype; a, b: label tensors of that shape (any float dtype,
    read as float32; b is None for "ranknet" and "margin"); kind: a key of PAIR_KINDS or its value.  loss is the mean over
    the elements, the gradients include the 1 / n.  One launch up to 4,096 elements, two above; on the current stream, no
    read-back: graph-capturable."""
    kind = _kind(PAIR_KINDS, kind, "pair_loss")
    dev = _dev_check(pos, neg, a, b)
    if pos.dtype not in _DT or neg.dtype != pos.dtype or neg.shape != pos.shape:
        raise NativeError(f"pair_loss: pos and neg must be float32 / float16 / bfloat16 of one shape and dtype, got "
                          f"{pos.dtype} {tuple(pos.shape)} and {neg.dtype} {tuple(neg.shape)}")
    if a is None or (b is None and kind not in _ONE_LABEL):
        raise NativeError("pair_loss: this kind needs " + ("label a" if a is None else "labels a and b"), _lib.MM_EINVAL)
    n = pos.numel()
    if n > 1 << 31:
        raise NativeError(f"pair_loss: n={n} > 2^31", _lib.MM_EUNSUPPORTED)
    pos_c, neg_c = pos.detach().contiguous(), neg.detach().contiguous()
    a = _label32(a, pos.shape, "pair_loss", "a")
    b = _label32(b, pos.shape, "pair_loss", "b") if b is not None and kind not in _ONE_LABEL else None
    loss = torch.empty((), dtype=torch.float32, device=dev)
    gpos = torch.empty(pos.shape, dtype=pos.dtype, device=dev)
    gneg = torch.empty(pos.shape, dtype=pos.dtype, device=dev)
    L = _lib.lib()
    wsb = ops._ws_bytes(L.mm_pair_loss_workspace_bytes, n)
    ws = _workspace(dev, wsb)
    _call(dev, L.mm_pair_loss_fwd, (pos_c.data_ptr(), neg_c.data_ptr(), _DT[pos.dtype], a.data_ptr(),
                                    b.data_ptr() if b is not None else None, n, kind, loss.data_ptr(), gpos.data_ptr(),
                                    gneg.data_ptr(), ws.data_ptr() if ws is not None else None, wsb), stream_only=True)
    return loss, gpos, gneg


def list_loss(scores, labels, kind):
    """(loss [] float32, per_list [B] float32, grad [B, L] like scores) of a listwise loss (native mm_list_loss_fwd).

    scores [B, L] float32 / float16 / bfloat16, labels [B, L] (read as float32), L <= MAX_LIST (more raises NativeError with
    .code == MM_EUNSUPPORTED: the caller takes another route); kind: a key of LIST_KINDS or its value.  per_list is the list's
    own term before the batch reduction (a mean over B; a sum for the Lambda kinds).  Neither input is modified.  Two launches
    on the current stream, no workspace, no read-back: graph-capturable."""
    kind = _kind(LIST_KINDS, kind, "list_loss")
    dev = _dev_check(scores, labels)
    if scores.dim() != 2 or scores.dtype not in _DT:
        raise NativeError(f"list_loss: scores must be float32 / float16 / bfloat16 [B, L], got {scores.dtype} {tuple(scores.shape)}")
    B, Ln = scores.shape
    if Ln > MAX_LIST:
        raise NativeError(f"list_loss: L={Ln} above the native limit of {MAX_LIST} entries per list", _lib.MM_EUNSUPPORTED)
    if B >= 1 << 31:
        raise NativeError(f"list_loss: B={B} >= 2^31", _lib.MM_EUNSUPPORTED)
    sc = scores.detach().contiguous()
    labels = _label32(labels, scores.shape, "list_loss", "labels")
    loss = torch.empty((), dtype=torch.float32, device=dev)
    per_list = torch.empty(B, dtype=torch.float32, device=dev)
    grad = torch.empty((B, Ln), dtype=scores.dtype, device=dev)
    _call(dev, _lib.lib().mm_list_loss_fwd, (sc.data_ptr(), _DT[scores.dtype], labels.data_ptr(), B, Ln, kind, loss.data_ptr(),
                                             per_list.data_ptr(), grad.data_ptr()), stream_only=True)
    return loss, per_list, grad


def list_loss_backward(grad, kind, g_loss, g_per_list):
    """grad_scores from the saved gradient: grad x grad_output of the loss, plus grad x B x grad_output of per_list (the saved
    rows carry the 1 / B of the mean; the Lambda kinds sum, so their rows are per_list's own)."""
    out = None
    if g_loss is not None:
        out = grad * g_loss
    if g_per_list is not None:
        scale = 1 if kind in _SUM_KINDS else grad.shape[0]
        t = grad * (g_per_list * scale).to(grad.dtype)[:, None]
        out = t if out is None else out + t
    return out


class _PairLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, neg, a, b, kind):
        loss, gpos, gneg = pair_loss(pos, neg, a, b, kind)
        ctx.save_for_backward(gpos, gneg)
        return loss

    @staticmethod
    def backward(ctx, g):
        gpos, gneg = ctx.saved_tensors
        return (gpos * g if ctx.needs_input_grad[0] else None), (gneg * g if ctx.needs_input_grad[1] else None), None, None, None


class _ListLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, labels, kind):
        loss, per_list, grad = list_loss(scores, labels, kind)
        ctx.save_for_backward(grad)
        ctx.kind = LIST_KINDS.get(kind, kind)
        ctx.set_materialize_grads(False)      # an unused output's gradient stays None: no multiply by zeros
        return loss, per_list

    @staticmethod
    def backward(ctx, g_loss, g_per_list):
        return list_loss_backward(ctx.saved_tensors[0], ctx.kind, g_loss, g_per_list), None, None


# ---- the route -------------------------------------------------------------------------------------------------------------
def _native_scores(*scores):
    s0 = scores[0]
    return all(isinstance(s, torch.Tensor) and s.is_cuda and s.dtype in _DT and s.dtype == s0.dtype and s.shape == s0.shape
               and s.device == s0.device for s in scores)


def _native_labels(s0, *labels):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == s0.device and t.shape == s0.shape
               and t.is_floating_point() and not t.requires_grad for t in labels)


def _pair_route(mod, pos, neg, *labels):
    return bool(mod.native) and _native_scores(pos, neg) and _native_labels(pos, *labels) and pos.numel() <= 1 << 31


def _list_route(mod, scores, labels):
    return (bool(mod.native) and _native_scores(scores) and _native_labels(scores, labels) and scores.dim() == 2
            and scores.shape[0] > 0 and 0 < scores.shape[1] <= MAX_LIST)


# ---- drop-in classes: pairwise / pointwise -----------------------------------------------------------------------------------
class MSMarginLoss(nn.Module):
    """Margin-MSE (matchmaker/losses/msmargin.py:4-14): the mean squared difference of the score margin and the label margin.
    native defaults to False: 1.13-1.34 x faster than eager in every leg of three measured runs, but in two legs of one run inside
    the spread of its two rounds (DESIGN 3.22's rule); `loss.native = True` selects the kernel."""
    native = False

    def __init__(self):
        super().__init__()

    def eager(self, scores_pos, scores_neg, label_pos, label_neg):
        return torch.mean(torch.pow((scores_pos - scores_neg) - (label_pos - label_neg), 2))

    def forward(self, scores_pos, scores_neg, label_pos, label_neg):
        if _pair_route(self, scores_pos, scores_neg, label_pos, label_neg):
            return _PairLoss.apply(scores_pos, scores_neg, label_pos, label_neg, _lib.PAIR_MARGIN_MSE)
        return self.eager(scores_pos, scores_neg, label_pos, label_neg)


class MSETeacherPointwise(nn.Module):
    """(MSE(pos, label_pos) + MSE(neg, label_neg)) / 2 (matchmaker/losses/teacher_mse_pointwise.py:4-14)."""
    native = True

    def __init__(self):
        super().__init__()
        self.mse = torch.nn.MSELoss()

    def eager(self, scores_pos, scores_neg, label_pos, label_neg):
        return (self.mse(scores_pos, label_pos) + self.mse(scores_neg, label_neg)) / 2

    def forward(self, scores_pos, scores_neg, label_pos, label_neg):
        if _pair_route(self, scores_pos, scores_neg, label_pos, label_neg):
            return _PairLoss.apply(scores_pos, scores_neg, label_pos, label_neg, _lib.PAIR_MSE_POINTWISE)
        return self.eager(scores_pos, scores_neg, label_pos, label_neg)


class KLDivTeacherPointwise(nn.Module):
    """(KLDivLoss()(pos, label_pos) + KLDivLoss()(neg, label_neg)) / 2 on raw scores, as the reference has it
    (matchmaker/losses/teacher_kldiv_pointwise.py:4-14): the element-wise mean of xlogy(t, t) - t x."""
    native = True

    def __init__(self):
        super().__init__()

    @staticmethod
    def _kl(x, t):
        return (torch.xlogy(t, t) - t * x).mean()

    def eager(self, scores_pos, scores_neg, label_pos, label_neg):
        return (self._kl(scores_pos, label_pos) + self._kl(scores_neg, label_neg)) / 2

    def forward(self, scores_pos, scores_neg, label_pos, label_neg):
        if _pair_route(self, scores_pos, scores_neg, label_pos, label_neg):
            return _PairLoss.apply(scores_pos, scores_neg, label_pos, label_neg, _lib.PAIR_KLDIV_POINTWISE)
        return self.eager(scores_pos, scores_neg, label_pos, label_neg)


class RankNetTeacher(nn.Module):
    """RankNet towards 1, weighted by the teacher's margin (matchmaker/losses/teacher_ranknetweighted.py:6-19)."""
    native = True

    def __init__(self):
        super().__init__()

    def eager(self, scores_pos, scores_neg, label_pos, label_neg):
        x = scores_pos - scores_neg
        return F.binary_cross_entropy_with_logits(x, torch.ones_like(x), weight=label_pos - label_neg)

    def forward(self, scores_pos, scores_neg, label_pos, label_neg):
        if _pair_route(self, scores_pos, scores_neg, label_pos, label_neg):
            return _PairLoss.apply(scores_pos, scores_neg, label_pos, label_neg, _lib.PAIR_RANKNET_TEACHER)
        return self.eager(scores_pos, scores_neg, label_pos, label_neg)


class MSERanknetTeacher(nn.Module):
    """MSETeacherPointwise + RankNet towards 1 (matchmaker/losses/teacher_mse_ranknet.py:4-15)."""
    native = True

    def __init__(self):
        super().__init__()
        self.mse = torch.nn.MSELoss()

    def eager(self, scores_pos, scores_neg, label_pos, label_neg):
        x = scores_pos - scores_neg
        pointwise = (self.mse(scores_pos, label_pos) + self.mse(scores_neg, label_neg)) / 2
        return pointwise + F.binary_cross_entropy_with_logits(x, torch.ones_like(x))

    def forward(self, scores_pos, scores_neg, label_pos, label_neg):
        if _pair_route(self, scores_pos, scores_neg, label_pos, label_neg):
            return _PairLoss.apply(scores_pos, scores_neg, label_pos, label_neg, _lib.PAIR_MSE_RANKNET)
        return self.eager(scores_pos, scores_neg, label_pos, label_neg)


class RankNetLoss(nn.Module):
    """BCEWithLogits(pos - neg, probs) (matchmaker/losses/ranknet.py:4-17).  native defaults to False: 1.23-1.46 x faster than
    eager in every leg of three measured runs, but each run had one leg with a slow round inside eager's range (DESIGN 3.22's rule)."""
    native = False

    def __init__(self):
        super().__init__()
        self.bce = torch.nn.BCEWithLogitsLoss()

    def eager(self, scores_pos, scores_neg, probs):
        return self.bce(scores_pos - scores_neg, probs)

    def forward(self, scores_pos, scores_neg, probs):
        if _pair_route(self, scores_pos, scores_neg, probs):
            return _PairLoss.apply(scores_pos, scores_neg, probs, None, _lib.PAIR_RANKNET)
        return self.eager(scores_pos, scores_neg, probs)


class MarginRankingLoss1(torch.nn.MarginRankingLoss):
    """torch.nn.MarginRankingLoss(margin=1, reduction="mean"), what get_loss returns for "margin"
    (matchmaker/losses/all.py:48)."""
    native = True

    def __init__(self):
        super().__init__(margin=1, reduction="mean")

    def eager(self, input1, input2, target):
        return F.margin_ranking_loss(input1, input2, target, margin=self.margin, reduction=self.reduction)

    def forward(self, input1, input2, target):
        if self.margin == 1 and self.reduction == "mean" and _pair_route(self, input1, input2, target):
            return _PairLoss.apply(input1, input2, target, None, _lib.PAIR_MARGIN)
        return self.eager(input1, input2, target)


# ---- drop-in classes: listwise ---------------------------------------------------------------------------------------------
class SmoothRank(nn.Module):
    """rank_i = 0.5 + sum_j sigmoid(s_j - s_i) (matchmaker/losses/loss_smooth_mrr.py:4-16)."""

    def __init__(self):
        super().__init__()
        self.sigmoid = torch.nn.Sigmoid()

    def forward(self, scores):
        return torch.sum(self.sigmoid(scores.unsqueeze(-2) - scores.unsqueeze(-1)), dim=-1) + 0.5


class SmoothMRRLoss(nn.Module):
    """1 - max_i [label_i > 0] / rank_i per list, the mean over the lists unless agg=False
    (matchmaker/losses/loss_smooth_mrr.py:18-34).  Native route: the gradient flows through the lowest arg-max index."""
    native = True

    def __init__(self):
        super().__init__()
        self.soft_ranker = SmoothRank()
        self.zero = nn.Parameter(torch.tensor([0], dtype=torch.float32), requires_grad=False)
        self.one = nn.Parameter(torch.tensor([1], dtype=torch.float32), requires_grad=False)

    def eager(self, scores, labels, agg=True):
        rr = torch.where(labels > 0, self.one, self.zero) / self.soft_ranker(scores)
        loss = 1 - rr.max(dim=-1)[0]
        return loss.mean() if agg else loss

    def forward(self, scores, labels, agg=True):
        if _list_route(self, scores, labels):
            loss, per_list = _ListLoss.apply(scores, labels, _lib.LIST_SMOOTH_MRR)
            return loss if agg else per_list
        return self.eager(scores, labels, agg)


class ListNetLoss(nn.Module):
    """-sum_i softmax(y_true)_i log(softmax(y_pred)_i + eps), the mean over the lists (matchmaker/losses/listnet.py:5-33)."""
    native = True

    def __init__(self):
        super().__init__()

    def eager(self, y_pred, y_true, eps=1e-6):
        return torch.mean(-torch.sum(F.softmax(y_true, dim=1) * torch.log(F.softmax(y_pred, dim=1) + eps), dim=1))

    def forward(self, y_pred, y_true, eps=1e-6):
        if eps == 1e-6 and _list_route(self, y_pred, y_true):
            return _ListLoss.apply(y_pred, y_true, _lib.LIST_LISTNET)[0]
        return self.eager(y_pred, y_true, eps)


class KLDivTeacherList(nn.Module):
    """KLDivLoss("batchmean") fed softmax(scores) and softmax(labels), as the reference has it
    (matchmaker/losses/teacher_kldiv_list.py:4-14): sum(xlogy(T, T) - T p) / B."""
    native = True

    def __init__(self):
        super().__init__()

    def eager(self, scores, labels):
        p, t = scores.softmax(-1), labels.softmax(-1)
        return (torch.xlogy(t, t) - t * p).sum() / p.shape[0]

    def forward(self, scores, labels):
        if _list_route(self, scores, labels):
            return _ListLoss.apply(scores, labels, _lib.LIST_KLDIV)[0]
        return self.eager(scores, labels)


DEFAULT_EPS = 1e-6


def _inv(t):
    return torch.pow(torch.abs(t), -1.)


def _w_ndcg1(G, D, mu, t):
    return (G / D)[:, :, None]


def _w_ndcg2(G, D, mu=None, t=None):
    pos = torch.arange(1, G.shape[1] + 1, device=G.device)
    gap = torch.abs(pos[:, None] - pos[None, :])
    delta = torch.abs(_inv(D[0, gap - 1]) - _inv(D[0, gap]))
    delta.diagonal().zero_()
    return delta[None, :, :] * torch.abs(G[:, :, None] - G[:, None, :])


def _w_lambdarank(G, D, mu=None, t=None):
    return torch.abs(torch.pow(D[:, :, None], -1.) - torch.pow(D[:, None, :], -1.)) * torch.abs(G[:, :, None] - G[:, None, :])


def _w_ndcg2pp(G, D, mu, t):
    return mu * _w_ndcg2(G, D) + _w_lambdarank(G, D)


_SCHEMES = {
    "ndcgLoss1_scheme": _w_ndcg1,
    "ndcgLoss2_scheme": _w_ndcg2,
    "lamdbaRank_scheme": _w_lambdarank,      # (the reference's spelling)
    "ndcgLoss2PP_scheme": _w_ndcg2pp,
    "rankNet_scheme": lambda G, D, mu, t: 1.,
    "rankNetWeightedByGTDiff_scheme": lambda G, D, mu, t: torch.abs(t[:, :, None] - t[:, None, :]),
    "rankNetWeightedByGTDiffPowed_scheme": lambda G, D, mu, t: torch.abs(torch.pow(t[:, :, None], 2) - torch.pow(t[:, None, :], 2)),
}


class LambdaLoss(nn.Module):
    """The LambdaLoss framework (matchmaker/losses/lambdarank.py:38-119, after allRank's lambdaLoss).  The native route covers
    what get_loss uses: weighing_scheme "ndcgLoss2_scheme" with every forward argument at its default.  STATED CHOICE: neither
    route modifies its inputs (the reference writes -inf into y_pred and y_true in place)."""
    native = True

    def __init__(self, weighing_scheme=None):
        super().__init__()
        self.weighing_scheme = weighing_scheme

    def eager(self, y_pred, y_true, padded_value_indicator=-1, eps=DEFAULT_EPS, k=None, sigma=1., mu=10., reduction="sum",
              reduction_log="binary"):
        if reduction_log not in ("natural", "binary"):
            raise ValueError("Reduction logarithm base can be either natural or binary")
        if reduction not in ("sum", "mean"):
            raise ValueError("Reduction method can be either sum or mean")
        if self.weighing_scheme is not None and self.weighing_scheme not in _SCHEMES:
            raise KeyError(self.weighing_scheme)
        dev, n = y_pred.device, y_pred.shape[1]
        padded = y_true == padded_value_indicator
        y_pred = y_pred.masked_fill(padded, float("-inf"))
        y_true = y_true.masked_fill(padded, float("-inf"))
        pred_sorted, order = y_pred.sort(descending=True, stable=True, dim=-1)      # ties in arrival order, as the kernel
        true_sorted = y_true.sort(descending=True, dim=-1)[0]
        t = torch.gather(y_true, dim=1, index=order)
        diffs = t[:, :, None] - t[:, None, :]
        counted = torch.isfinite(diffs)
        if self.weighing_scheme != "ndcgLoss1_scheme":
            counted = counted & (diffs > 0)
        top_k = torch.zeros((n, n), dtype=torch.bool, device=dev)
        top_k[:k, :k] = 1
        t = t.clamp(min=0.)
        true_sorted = true_sorted.clamp(min=0.)
        D = torch.log2(1. + torch.arange(1, n + 1, device=dev).float())[None, :]
        max_dcg = torch.sum(((torch.pow(2, true_sorted) - 1) / D)[:, :k], dim=-1).clamp(min=eps)
        G = (torch.pow(2, t) - 1) / max_dcg[:, None]
        weights = 1. if self.weighing_scheme is None else _SCHEMES[self.weighing_scheme](G, D, mu, t)
        x = (pred_sorted[:, :, None] - pred_sorted[:, None, :]).clamp(min=-1e4, max=1e4)
        x = x.masked_fill(torch.isnan(x), 0.)
        probs = (torch.sigmoid(sigma * x).clamp(min=eps) ** weights).clamp(min=eps)
        terms = (torch.log(probs) if reduction_log == "natural" else torch.log2(probs))[counted & top_k]
        return -torch.sum(terms) if reduction == "sum" else -torch.mean(terms)

    def _native_args(self, padded_value_indicator, eps, k, sigma, reduction, reduction_log):
        return (self.weighing_scheme == "ndcgLoss2_scheme" and padded_value_indicator == -1 and eps == DEFAULT_EPS and k is None
                and sigma == 1. and reduction == "sum" and reduction_log == "binary")

    def forward(self, y_pred, y_true, padded_value_indicator=-1, eps=DEFAULT_EPS, k=None, sigma=1., mu=10., reduction="sum",
                reduction_log="binary"):
        if self._native_args(padded_value_indicator, eps, k, sigma, reduction, reduction_log) and _list_route(self, y_pred, y_true):
            return _ListLoss.apply(y_pred, y_true, _lib.LIST_LAMBDA_NDCG2)[0]
        return self.eager(y_pred, y_true, padded_value_indicator, eps, k, sigma, mu, reduction, reduction_log)


class LambdaLossTeacher(LambdaLoss):
    """LambdaLoss on teacher scores: labels <- softmax(labels), + 2 where > 0.001 (matchmaker/losses/lambdarank.py:122-134)."""

    def __init__(self, weighing_scheme=None):
        super().__init__(weighing_scheme)

    def eager(self, y_pred, y_true):      # noqa: D102  (the reference's narrower signature)
        y_true = y_true.softmax(-1)
        y_true = torch.where(y_true > 0.001, y_true + 2, y_true)
        return LambdaLoss.eager(self, y_pred, y_true.detach())

    def forward(self, y_pred, y_true):
        if self.weighing_scheme == "ndcgLoss2_scheme" and _list_route(self, y_pred, y_true):
            return _ListLoss.apply(y_pred, y_true, _lib.LIST_LAMBDA_NDCG2_TEACHER)[0]
        return self.eager(y_pred, y_true)


# ---- get_loss ----------------------------------------------------------------------------------------------------------------
def _reference_loss(name):
    """(class, None) of a loss this package does not restate, from the reference; (None, why) when the reference cannot be
    imported or does not define it.  Any other error inside the reference propagates."""
    import importlib
    try:
        return getattr(importlib.import_module("matchmaker.losses.all"), name), None
    except (ImportError, AttributeError) as e:
        return None, f"{type(e).__name__}: {e}"


def get_loss(config):
    """(loss, qa_loss, inbatch_loss, use_list_loss, use_inbatch_list_loss) from the keys matchmaker/losses/all.py:23-86 reads,
    built from the classes of this module.  MSETeacherPointwisePassages, MarginMSE_InterPassageLoss and the QA loss come from
    the reference when it is importable; without it they raise, naming the loss."""
    use_list_loss = use_inbatch_list_loss = False
    qa_loss = inbatch_loss = None
    name = config["loss"]
    plain = {"margin-mse": MSMarginLoss, "MSETeacherPointwise": MSETeacherPointwise, "KLDivTeacherPointwise": KLDivTeacherPointwise,
             "RankNetTeacher": RankNetTeacher, "MSERanknetTeacher": MSERanknetTeacher, "ranknet": RankNetLoss,
             "margin": MarginRankingLoss1}
    lists = {"mrr": SmoothMRRLoss, "listnet": ListNetLoss, "lambdarank": lambda: LambdaLoss("ndcgLoss2_scheme")}
    if name in plain:
        loss = plain[name]()
    elif name in lists:
        loss, use_list_loss = lists[name](), True
    elif name in ("MSETeacherPointwisePassages", "MarginMSE_InterPassageLoss"):
        cls, why = _reference_loss(name)
        if cls is None:
            raise Exception(f"Loss not known: {name} is not restated by matchmaker_amd and the reference does not supply it ({why})")
        loss = cls()
    else:
        raise Exception(f"Loss not known: {name}")

    if config["train_qa_spans"]:
        cls, why = _reference_loss("QA_StartEndCrossEntropy") if config["qa_loss"] == "StartEndCrossEntropy" else (None, "no such QA loss")
        if cls is None:
            raise Exception(f"QA-Loss not known, qa_loss must be set with train_qa_spans: {config['qa_loss']} ({why})")
        qa_loss = cls()

    if config["in_batch_negatives"]:
        ib = config["in_batch_neg_loss"]
        if ib == "ranknet":
            inbatch_loss = RankNetLoss()
        elif ib == "margin-mse":
            inbatch_loss = MSMarginLoss()
        elif ib in ("KLDivTeacherList", "listnet", "lambdarank"):
            inbatch_loss = {"KLDivTeacherList": KLDivTeacherList, "listnet": ListNetLoss,
                            "lambdarank": lambda: LambdaLossTeacher("ndcgLoss2_scheme")}[ib]()
            use_inbatch_list_loss = True
        else:
            raise Exception(f"In-batch-Loss not known, in_batch_neg_loss must be set with in_batch_negatives: {ib}")
    return loss, qa_loss, inbatch_loss, use_list_loss, use_inbatch_list_loss


__all__ = ["pair_loss", "list_loss", "get_loss", "MAX_LIST", "PAIR_KINDS", "LIST_KINDS", "MSMarginLoss", "MSETeacherPointwise",
           "KLDivTeacherPointwise", "RankNetTeacher", "MSERanknetTeacher", "RankNetLoss", "MarginRankingLoss1", "SmoothRank",
           "SmoothMRRLoss", "ListNetLoss", "KLDivTeacherList", "LambdaLoss", "LambdaLossTeacher"]
