"""In-batch negatives of dense-retriever training (matchmaker/train.py:434-472; BERT_DOT under TAS-Balanced, ColBERT through
its all-pairs score matrices) over two fused operators of libmm_native.so (csrc/inbatch_loss.hip):

    inbatch_dot_loss(Q, Dp, Dn, sp, Tp, Tn, family, kind)     -> (loss, stats, grad_Q, grad_Dp, grad_Dn, grad_sp)   mm_inbatch_dot_loss_fwd
    inbatch_select_loss(sp, Sp, Sn, Tp, Tn, family, kind)    -> (loss, stats, grad_sp, grad_Sp, grad_Sn)           mm_inbatch_select_loss_fwd

Each call returns the in-batch loss, its three statistics AND every gradient, so autograd's backward is one multiply by
grad_output per input.  `InBatchNegatives` is the module train.py's block becomes (INTEGRATION.md shows the edit): it maps the
configured in-batch loss object to (family, kind) by its class, and holds its own eager formula, which runs for CPU tensors,
unsupported shapes and dtypes, teacher tensors that require grad and loss objects it does not know.  A call that takes the native
route and fails raises: nothing falls back after the decision.

The torch <-> ABI wrappers live here, not in ops.py (ops.inbatch_dot_loss forwards); the module has its own `torch`, `_workspace`
and `clear_workspaces` names and allocates its outputs with `torch.empty`, so tests/poison.py can be pointed at it.
"""
import torch
import torch.nn as nn

from . import _lib, losses, ops
from ._lib import NativeError
from .ops import _DT, _call, _dev_check, _workspace, clear_workspaces  # noqa: F401  (re-exported: tests/poison.py patches them here)

PAIR, LIST = _lib.INBATCH_PAIR, _lib.INBATCH_LIST
FAMILIES = {"pair": PAIR, "list": LIST}
MAX_B = 1024            # rows of a native call (the list family: 2 B <= losses.MAX_LIST)
MIN_E, MAX_E = 8, 1024
_ONE_LABEL = (_lib.PAIR_RANKNET, _lib.PAIR_MARGIN)

# a family's default is True only if the slowest native round beat the fastest eager round in every leg of every
# measured run (tools/bench_inbatch_loss.py).  Three runs, 42 legs each: every leg of both families, by 1.8 x at the least.
NATIVE_DEFAULT = {PAIR: True, LIST: True}


def _family_kind(family, kind, op):
    fam = FAMILIES.get(family, family) if isinstance(family, str) else family
    if fam not in (PAIR, LIST):
        raise NativeError(f"{op}: unknown family {family!r} (\"pair\" or \"list\")", _lib.MM_EINVAL)
    return fam, losses._kind(losses.PAIR_KINDS if fam == PAIR else losses.LIST_KINDS, kind, op)


def _teacher32(t, B, op, name):
    if t is None:
        return None
    if tuple(t.shape) != (B, B):
        raise NativeError(f"{op}: {name} has shape {tuple(t.shape)}, expected {(B, B)}")
    return t.detach().to(torch.float32).contiguous()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _rows16(t):
    """t detached and contiguous at a 16-byte aligned address (the scores kernel loads 16 bytes per lane): a contiguous view at
    another storage offset is copied"""
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


# ---- torch <-> ABI ---------------------------------------------------------------------------------------------------------
def inbatch_select_loss(sp, Sp, Sn, Tp, Tn, family, kind):
    """(loss [] float32, stats [3] float32, grad_sp [B], grad_Sp, grad_Sn [B, B] like the scores) of the in-batch negatives over
    score matrices (native mm_inbatch_select_loss_fwd; train.py:434-438, :443-472).

    sp [B] = the paired positive scores, Sp, Sn [B, B] = the query x positive / negative document scores, one dtype of float32 /
    float16 / bfloat16; Tp, Tn [B, B] teacher scores (read as float32) or both None; family "pair" | "list", kind a key (or value)
    of losses.PAIR_KINDS / losses.LIST_KINDS.  stats = (accuracy, score_diff, teacher accuracy or NaN).  Two launches (three for
    the list family) on the current stream, no read-back: graph-capturable."""
    op = "inbatch_select_loss"
    family, kind = _family_kind(family, kind, op)
    dev = _dev_check(sp, Sp, Sn, Tp, Tn)
    if (Sp.dim() != 2 or Sp.shape[0] != Sp.shape[1] or Sn.shape != Sp.shape or sp.shape != Sp.shape[:1] or Sp.dtype not in _DT
            or Sn.dtype != Sp.dtype or sp.dtype != Sp.dtype):
        raise NativeError(f"{op}: sp [B], Sp, Sn [B, B] must be float32 / float16 / bfloat16 of one dtype, got {sp.dtype} "
                          f"{tuple(sp.shape)}, {Sp.dtype} {tuple(Sp.shape)}, {Sn.dtype} {tuple(Sn.shape)}")
    B = Sp.shape[0]
    sp_c, Sp_c, Sn_c = sp.detach().contiguous(), Sp.detach().contiguous(), Sn.detach().contiguous()
    Tp, Tn = _teacher32(Tp, B, op, "Tp"), _teacher32(Tn, B, op, "Tn")
    loss = torch.empty((), dtype=torch.float32, device=dev)
    stats = torch.empty(3, dtype=torch.float32, device=dev)
    gsp = torch.empty(B, dtype=Sp.dtype, device=dev)
    gSp = torch.empty((B, B), dtype=Sp.dtype, device=dev)
    gSn = torch.empty((B, B), dtype=Sp.dtype, device=dev)
    L = _lib.lib()
    wsb = ops._ws_bytes(L.mm_inbatch_select_loss_workspace_bytes, B, family)
    ws = _workspace(dev, wsb)
    _call(dev, L.mm_inbatch_select_loss_fwd, (sp_c.data_ptr(), Sp_c.data_ptr(), Sn_c.data_ptr(), _DT[Sp.dtype], _ptr(Tp), _ptr(Tn), B,
                                              family, kind, loss.data_ptr(), stats.data_ptr(), gsp.data_ptr(), gSp.data_ptr(),
                                              gSn.data_ptr(), _ptr(ws), wsb), stream_only=True)
    return loss, stats, gsp, gSp, gSn


def inbatch_dot_loss(Q, Dp, Dn, sp, Tp, Tn, family, kind, need_grad=True, return_scores=False):
    """(loss [] float32, stats [3] float32, grad_Q, grad_Dp, grad_Dn [B, E] like the vectors, grad_sp [B] like sp) of the in-batch
    negatives from the vectors (native mm_inbatch_dot_loss_fwd; train.py:434-472 with its two torch.mm and its backward).

    Q, Dp, Dn [B, E]: query, positive and negative document vectors of one dtype (float32 / float16 / bfloat16); sp [B] the
    paired positive scores in a dtype of its own; Tp, Tn [B, B] teacher scores or both None; family, kind as inbatch_select_loss.
    The scores are formed and kept in float32 (STATED CHOICE, include/mm_native.h).  need_grad=False: loss and statistics only,
    the four gradients are None and the gradient launch is skipped.  return_scores=True appends copies of the float32 score
    matrices (Sp, Sn) the call formed.  1 <= B <= MAX_B (list family: 2 B <= losses.MAX_LIST), MIN_E <= E <= MAX_E, rows of 16
    bytes; anything else raises NativeError with .code == MM_EUNSUPPORTED.  Three launches (four for the list family) on the
    current stream, no read-back: graph-capturable."""
    op = "inbatch_dot_loss"
    family, kind = _family_kind(family, kind, op)
    dev = _dev_check(Q, Dp, Dn, sp, Tp, Tn)
    if (Q.dim() != 2 or Dp.shape != Q.shape or Dn.shape != Q.shape or Q.dtype not in _DT or Dp.dtype != Q.dtype or Dn.dtype != Q.dtype
            or sp.shape != Q.shape[:1] or sp.dtype not in _DT):
        raise NativeError(f"{op}: Q, Dp, Dn [B, E] must be float32 / float16 / bfloat16 of one dtype and sp [B], got {Q.dtype} "
                          f"{tuple(Q.shape)}, {Dp.dtype} {tuple(Dp.shape)}, {Dn.dtype} {tuple(Dn.shape)}, {sp.dtype} {tuple(sp.shape)}")
    B, E = Q.shape
    Q_c, Dp_c, Dn_c, sp_c = _rows16(Q), _rows16(Dp), _rows16(Dn), sp.detach().contiguous()
    Tp, Tn = _teacher32(Tp, B, op, "Tp"), _teacher32(Tn, B, op, "Tn")
    loss = torch.empty((), dtype=torch.float32, device=dev)
    stats = torch.empty(3, dtype=torch.float32, device=dev)
    gQ = gDp = gDn = gsp = None
    if need_grad:
        gQ = torch.empty((B, E), dtype=Q.dtype, device=dev)
        gDp = torch.empty((B, E), dtype=Q.dtype, device=dev)
        gDn = torch.empty((B, E), dtype=Q.dtype, device=dev)
        gsp = torch.empty(B, dtype=sp.dtype, device=dev)
    L = _lib.lib()
    wsb = ops._ws_bytes(L.mm_inbatch_dot_loss_workspace_bytes, B, E, family)
    ws = _workspace(dev, wsb)
    _call(dev, L.mm_inbatch_dot_loss_fwd, (Q_c.data_ptr(), Dp_c.data_ptr(), Dn_c.data_ptr(), _DT[Q.dtype], sp_c.data_ptr(),
                                           _DT[sp.dtype], _ptr(Tp), _ptr(Tn), B, E, family, kind, loss.data_ptr(), stats.data_ptr(),
                                           _ptr(gQ), _ptr(gDp), _ptr(gDn), _ptr(gsp), _ptr(ws), wsb), stream_only=True)
    out = (loss, stats, gQ, gDp, gDn, gsp)
    if return_scores:      # the workspace begins with Sp, Sn [2][B][B] float32
        S = ws[:8 * B * B].view(torch.float32).view(2, B, B).clone() if B else torch.zeros((2, 0, 0), device=dev)
        out += (S[0], S[1])
    return out


def _scaled(grad, g, needed):
    """saved gradient x grad_output, formed in fp32 and rounded once: under a GradScaler grad_output is loss_scale x lambda in fp32,
    which need not fit the gradient's 16-bit type although the product does"""
    if not needed:
        return None
    return grad * g if grad.dtype == torch.float32 else (grad.float() * g).to(grad.dtype)


class _DotLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sp, Q, Dp, Dn, Tp, Tn, family, kind):
        need = any(ctx.needs_input_grad[:4])
        loss, stats, gQ, gDp, gDn, gsp = inbatch_dot_loss(Q, Dp, Dn, sp, Tp, Tn, family, kind, need_grad=need)
        if need:
            ctx.save_for_backward(gsp, gQ, gDp, gDn)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g, _gstats):
        return tuple(_scaled(t, g, ctx.needs_input_grad[i]) for i, t in enumerate(ctx.saved_tensors)) + (None,) * 4


class _SelectLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sp, Sp, Sn, Tp, Tn, family, kind):
        loss, stats, gsp, gSp, gSn = inbatch_select_loss(sp, Sp, Sn, Tp, Tn, family, kind)
        ctx.save_for_backward(gsp, gSp, gSn)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g, _gstats):
        return tuple(_scaled(t, g, ctx.needs_input_grad[i]) for i, t in enumerate(ctx.saved_tensors)) + (None,) * 4


# ---- loss object -> (family, kind) --------------------------------------------------------------------------------------------
# class name -> (family, kind), for the classes of matchmaker/losses/*.py and their drop-ins of matchmaker_amd.losses (the same names)
_BY_NAME = {"RankNetLoss": (PAIR, _lib.PAIR_RANKNET), "MSMarginLoss": (PAIR, _lib.PAIR_MARGIN_MSE),
            "MSETeacherPointwise": (PAIR, _lib.PAIR_MSE_POINTWISE), "KLDivTeacherPointwise": (PAIR, _lib.PAIR_KLDIV_POINTWISE),
            "RankNetTeacher": (PAIR, _lib.PAIR_RANKNET_TEACHER), "MSERanknetTeacher": (PAIR, _lib.PAIR_MSE_RANKNET),
            "KLDivTeacherList": (LIST, _lib.LIST_KLDIV), "ListNetLoss": (LIST, _lib.LIST_LISTNET),
            "SmoothMRRLoss": (LIST, _lib.LIST_SMOOTH_MRR), "LambdaLoss": (LIST, _lib.LIST_LAMBDA_NDCG2),
            "LambdaLossTeacher": (LIST, _lib.LIST_LAMBDA_NDCG2_TEACHER)}


def family_kind_of(loss_fn):
    """(family, kind) of a loss object by its class, or None for one the kernels do not implement: the classes of
    matchmaker.losses.*, those of matchmaker_amd.losses, and torch.nn.MarginRankingLoss(margin=1, reduction="mean").  The Lambda
    classes count with weighing_scheme "ndcgLoss2_scheme" only (what get_loss builds)."""
    cls = type(loss_fn)
    if isinstance(loss_fn, torch.nn.MarginRankingLoss):
        return (PAIR, _lib.PAIR_MARGIN) if loss_fn.margin == 1 and loss_fn.reduction == "mean" else None
    mod = cls.__module__ or ""
    if not (mod == losses.__name__ or mod.startswith("matchmaker.losses")):
        return None
    fk = _BY_NAME.get(cls.__name__)
    if fk is not None and cls.__name__.startswith("LambdaLoss") and getattr(loss_fn, "weighing_scheme", None) != "ndcgLoss2_scheme":
        return None
    return fk


def _teachers_ok(Tp, Tn, B, dev):
    if Tp is None and Tn is None:
        return True
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and tuple(t.shape) == (B, B) and t.is_floating_point()
               and not t.requires_grad for t in (Tp, Tn))


def _fits(fk, B, Tp):
    """whether the native entries take this (family, kind) at B rows with / without a teacher"""
    family, kind = fk
    if family == LIST:
        return Tp is not None and 1 <= B and 2 * B <= losses.MAX_LIST
    return 1 <= B <= MAX_B and (Tp is None) == (kind in _ONE_LABEL)


class InBatchNegatives(nn.Module):
    """The in-batch-negatives block of the training loop (matchmaker/train.py:434-472) as one module.

        ib = InBatchNegatives(inbatch_loss_fn, use_inbatch_list_loss)
        ib_loss, stats = ib(ranking_score_pos, query_vecs_pos, doc_vecs_pos, doc_vecs_neg, teacher_pos, teacher_neg)

    stats = {"accuracy", "score_diff", "teacher_accuracy"} (detached 0-dim tensors; teacher_accuracy is None without a teacher and
    for a list loss).  forward_scores takes the [B, B] score matrices instead of the vectors (ColBERT's all-pairs MaxSim).
    native: True / False, or None for the measured default of the loss's family (NATIVE_DEFAULT)."""

    def __init__(self, inbatch_loss_fn, use_inbatch_list_loss=False, native=None):
        super().__init__()
        self.inbatch_loss_fn = inbatch_loss_fn
        self.use_inbatch_list_loss = bool(use_inbatch_list_loss)
        fk = family_kind_of(inbatch_loss_fn)
        if fk is not None and (fk[0] == LIST) != self.use_inbatch_list_loss:      # a list loss in the pair call or the reverse
            fk = None
        self.family_kind = fk
        self.native = (fk is not None and NATIVE_DEFAULT[fk[0]]) if native is None else bool(native)

    # -- the eager formula -----------------------------------------------------------------------------------------------------
    def eager(self, sp, Sp, Sn, Tp=None, Tn=None):
        """(ib_loss, stats) from the score matrices with torch operators, in the order train.py:434-472 has them."""
        B = Sp.shape[0]
        off = ~torch.eye(B, dtype=torch.bool, device=Sp.device)
        pos = sp.unsqueeze(-1).expand(-1, B - 1).reshape(-1)      # sp_i once per in-batch partner
        ip, ineg = Sp[off], Sn[off]                               # row-major off-diagonal
        teacher_acc = None
        fn = self.inbatch_loss_fn
        if Tp is not None:
            if self.use_inbatch_list_loss:
                loss = fn(torch.cat([Sp, Sn], dim=1), torch.cat([Tp, Tn], dim=1))
            else:
                a = Tp[~off].unsqueeze(-1).expand(-1, B - 1).reshape(-1)
                bp, bn = Tp[off], Tn[off]
                loss = (fn(pos, ip, a, bp) + fn(pos, ineg, a, bn)) * 0.5
                teacher_acc = (((a > bp).float().mean() + (a > bn).float().mean()) * 0.5).detach()
        else:
            one = torch.ones(pos.shape[0], device=pos.device, dtype=pos.dtype)
            loss = (fn(pos, ip, one) + fn(pos, ineg, one)) * 0.5
        acc = (((pos > ip).float().mean() + (pos > ineg).float().mean()) * 0.5).detach()
        diff = (((pos - ip).mean() + (pos - ineg).mean()) * 0.5).detach()
        return loss, {"accuracy": acc, "score_diff": diff, "teacher_accuracy": teacher_acc}

    # -- routes ------------------------------------------------------------------------------------------------------------------
    def _stats(self, stats, Tp):
        pair_teacher = Tp is not None and self.family_kind[0] == PAIR
        return {"accuracy": stats[0], "score_diff": stats[1], "teacher_accuracy": stats[2] if pair_teacher else None}

    def _common(self, sp, B, dev, Tp, Tn):
        return (self.native and self.family_kind is not None and isinstance(sp, torch.Tensor) and sp.is_cuda and sp.device == dev
                and sp.dim() == 1 and sp.shape[0] == B and sp.dtype in _DT and _teachers_ok(Tp, Tn, B, dev)
                and _fits(self.family_kind, B, Tp))

    def dot_route(self, sp, Q, Dp, Dn, Tp=None, Tn=None):
        """whether forward() takes the native route for these arguments"""
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype in _DT for t in (Q, Dp, Dn)):
            return False
        B, E = Q.shape
        rows16 = E % (4 if Q.dtype == torch.float32 else 8) == 0
        return (Dp.shape == Q.shape and Dn.shape == Q.shape and Dp.dtype == Q.dtype and Dn.dtype == Q.dtype and Dp.device == Q.device
                and Dn.device == Q.device and MIN_E <= E <= MAX_E and rows16 and self._common(sp, B, Q.device, Tp, Tn))

    def scores_route(self, sp, Sp, Sn, Tp=None, Tn=None):
        """whether forward_scores() takes the native route for these arguments"""
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype in _DT for t in (Sp, Sn)):
            return False
        B = Sp.shape[0]
        return (Sp.shape == (B, B) and Sn.shape == (B, B) and Sn.dtype == Sp.dtype and Sn.device == Sp.device and isinstance(sp, torch.Tensor)
                and sp.dtype == Sp.dtype and self._common(sp, B, Sp.device, Tp, Tn))

    def forward(self, ranking_score_pos, query_vecs_pos, doc_vecs_pos, doc_vecs_neg, teacher_pos=None, teacher_neg=None):
        if self.dot_route(ranking_score_pos, query_vecs_pos, doc_vecs_pos, doc_vecs_neg, teacher_pos, teacher_neg):
            loss, stats = _DotLoss.apply(ranking_score_pos, query_vecs_pos, doc_vecs_pos, doc_vecs_neg, teacher_pos, teacher_neg,
                                         *self.family_kind)
            return loss, self._stats(stats, teacher_pos)
        Sp = torch.mm(query_vecs_pos, doc_vecs_pos.transpose(-2, -1))      # the query of the positive pair for both (train.py:439-440)
        Sn = torch.mm(query_vecs_pos, doc_vecs_neg.transpose(-2, -1))
        return self.eager(ranking_score_pos, Sp, Sn, teacher_pos, teacher_neg)

    def forward_scores(self, ranking_score_pos, Sp, Sn, teacher_pos=None, teacher_neg=None):
        if self.scores_route(ranking_score_pos, Sp, Sn, teacher_pos, teacher_neg):
            loss, stats = _SelectLoss.apply(ranking_score_pos, Sp, Sn, teacher_pos, teacher_neg, *self.family_kind)
            return loss, self._stats(stats, teacher_pos)
        return self.eager(ranking_score_pos, Sp, Sn, teacher_pos, teacher_neg)


__all__ = ["inbatch_dot_loss", "inbatch_select_loss", "InBatchNegatives", "family_kind_of", "FAMILIES", "NATIVE_DEFAULT", "MAX_B",
           "MIN_E", "MAX_E"]
