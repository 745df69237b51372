"""torch.ops.mm_native.* — the native operators as registered PyTorch custom ops.

Importing this module defines

    torch.ops.mm_native.maxsim(q, d, q_mask, d_mask, pairs_per_query=1,
                               sim_round=False, sum_round=False)                    -> [n_pairs]
    torch.ops.mm_native.maxsim_inbatch(q, q_mask, d, d_mask, bug_compatible=False,
                                       sim_round=False, sum_round=False)            -> [Bq, Bd]
    torch.ops.mm_native.kernel_pool(q, d, q_mask, d_mask, mu, sigma, alpha, w,
                                    pairs_per_query=1, d_gate=None, clamp_min=1e-10) -> [n_pairs]
    torch.ops.mm_native.tkl_window_pool(q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params,
                                        B, C, K, saturation)                        -> (score [B], windows [B, W])
    torch.ops.mm_native.colbert_candidates(hit_rows, begin_sorted, end_sorted, doc_of_sorted, T,
                                           c_cap=None)          -> (cand_doc, cand_begin, cand_end, count)
    torch.ops.mm_native.distinct_hits(scores, ids, top_n)        -> (scores, ids, pos, n_distinct, n_valid)
    torch.ops.mm_native.fp8_quantize_rows(x)                                       -> (codes [T, E] uint8, scales [T])
    torch.ops.mm_native.maxsim_ragged_fp8(q, codes, scales, doc_begin, doc_end, q_mask=None, pairs_per_query=1,
                                          check_ranges=True, sim_round=False, sum_round=False) -> [n_pairs]
    torch.ops.mm_native.segment_rank(scores, seg_begin, max_len)                    -> order [N] int32
    torch.ops.mm_native.pair_loss(pos, neg, a, b, kind)                             -> (loss [], grad_pos, grad_neg)
    torch.ops.mm_native.list_loss(scores, labels, kind)                             -> (loss [], per_list [B], grad [B, L])
    torch.ops.mm_native.inbatch_dot_loss(q, dp, dn, sp, tp, tn, family, kind)       -> (loss [], stats [3], grad_q, grad_dp, grad_dn, grad_sp)
    torch.ops.mm_native.inbatch_select_loss(sp, s_pos, s_neg, tp, tn, family, kind) -> (loss [], stats [3], grad_sp, grad_s_pos, grad_s_neg)
    torch.ops.mm_native.self_attention(qkv, mask, num_heads)                        -> out [B, L, E] (no autograd formula)

for HIP tensors only (dispatch key CUDA; a CPU tensor raises NotImplementedError: there is no CPU kernel), each
with a fake (meta) implementation for tracing, an autograd formula backed by the native backward kernels
(maxsim, maxsim_inbatch, kernel_pool; the two losses return their own gradient) and an autocast rule that mirrors what the reference's eager code does under
`torch.cuda.amp.autocast(enabled=use_fp16)` (colbert.py:60: the bmm runs in fp16 and RETURNS fp16 — the MaxSim ops cast
their vectors to the autocast dtype and set sim_round, so every per-token maximum is rounded as the reference's fp16 `max`
is — and the promoted `sum` returns fp32; the TK family stays fp32 — allennlp's cosine has no fp16 path the configs use, tk.yaml `use_fp16: False`).
The drop-in modules call `matchmaker_amd.ops` directly; these registrations are the boundary for callers
that want dispatcher-level ops (torch.compile graphs, TorchScript-free export, other extensions).
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import ops

_NS = "mm_native"


# ---------------------------------------------------------------------------------------------- maxsim
@torch.library.custom_op(_NS + "::maxsim", mutates_args=(), device_types="cuda")
def maxsim(q: Tensor, d: Tensor, q_mask: Optional[Tensor], d_mask: Optional[Tensor],
           pairs_per_query: int = 1, sim_round: bool = False, sum_round: bool = False) -> Tensor:
    return ops.maxsim(q, d, q_mask, d_mask, pairs_per_query, sim_round=sim_round, sum_round=sum_round)


@maxsim.register_fake
def _(q, d, q_mask, d_mask, pairs_per_query=1, sim_round=False, sum_round=False):
    return q.new_empty((d.shape[0],), dtype=torch.float32)


def _maxsim_setup(ctx, inputs, output):
    q, d, q_mask, d_mask, ppq, _sim, _sum = inputs
    ctx.save_for_backward(q, d, q_mask, d_mask)
    ctx.ppq = ppq


def _maxsim_backward(ctx, g):
    q, d, q_mask, d_mask = ctx.saved_tensors
    if ctx.ppq != 1:
        raise ops.NativeError("mm_native::maxsim backward needs the pair-per-row layout (pairs_per_query = 1), "
                              "the one train.py feeds")
    gq, gd = ops.maxsim_bwd(q, d, q_mask, d_mask, g, grad_dtype=q.dtype)
    return gq, gd, None, None, None, None, None


maxsim.register_autograd(_maxsim_backward, setup_context=_maxsim_setup)

_FRAG = torch.library.Library(_NS, "FRAGMENT")
_AUTOCAST_KEYS = torch._C.DispatchKeySet(torch._C.DispatchKey.AutocastCPU) | torch._C.DispatchKeySet(torch._C.DispatchKey.AutocastCUDA)


def _ac_cast(t):
    return t.to(torch.get_autocast_dtype("cuda")) if t.dtype == torch.float32 else t


def _maxsim_autocast(_ks, q, d, q_mask, d_mask, pairs_per_query=1, sim_round=False, sum_round=False):
    """What eager does under autocast (colbert.py:60-75): vectors in the autocast dtype, similarities and maxima in it
    (sim_round), the sum promoted to fp32."""
    with torch._C._ExcludeDispatchKeyGuard(_AUTOCAST_KEYS):
        return torch.ops.mm_native.maxsim(_ac_cast(q), _ac_cast(d), q_mask, d_mask, pairs_per_query, True, False)


_FRAG.impl("maxsim", _maxsim_autocast, "AutocastCUDA", with_keyset=True)


@torch.library.custom_op(_NS + "::maxsim_inbatch", mutates_args=(), device_types="cuda")
def maxsim_inbatch(q: Tensor, q_mask: Optional[Tensor], d: Tensor, d_mask: Optional[Tensor],
                   bug_compatible: bool = False, sim_round: bool = False, sum_round: bool = False) -> Tensor:
    return ops.maxsim_inbatch(q, q_mask, d, d_mask, bug_compatible, sim_round=sim_round, sum_round=sum_round)


@maxsim_inbatch.register_fake
def _(q, q_mask, d, d_mask, bug_compatible=False, sim_round=False, sum_round=False):
    return q.new_empty((q.shape[0], d.shape[0]), dtype=torch.float32)


@torch.library.custom_op(_NS + "::maxsim_inbatch_backward", mutates_args=(), device_types="cuda")
def maxsim_inbatch_backward(q: Tensor, q_mask: Optional[Tensor], d: Tensor, d_mask: Optional[Tensor], grad_out: Tensor,
                            bug_compatible: bool = False, need_q: bool = True, need_d: bool = True) -> Tuple[Tensor, Tensor]:
    """(grad_q, grad_d) of maxsim_inbatch in the token vectors' dtype (mm_maxsim_inbatch_bwd: first arg-max, fixed summation
    order, no atomics).  A gradient that is not needed is not computed: an empty tensor stands in its place."""
    gq, gd = ops.maxsim_inbatch_bwd(q, q_mask, d, d_mask, grad_out, bug_compatible, grad_dtype=q.dtype, need_q=need_q, need_d=need_d)
    return (gq if need_q else q.new_empty(0)), (gd if need_d else d.new_empty(0))


@maxsim_inbatch_backward.register_fake
def _(q, q_mask, d, d_mask, grad_out, bug_compatible=False, need_q=True, need_d=True):
    return q.new_empty(q.shape if need_q else 0), d.new_empty(d.shape if need_d else 0)


def _maxsim_inbatch_setup(ctx, inputs, output):
    q, q_mask, d, d_mask, bug_compatible, _sim, _sum = inputs
    ctx.save_for_backward(q, q_mask, d, d_mask)
    ctx.bug_compatible = bug_compatible


def _maxsim_inbatch_backward(ctx, g):
    """(the rounding flags are piecewise constant: the gradient is that of the unrounded maxima.  Under autocast the saved
    vectors are the cast ones, and autograd's own cast node hands fp32 leaves fp32 gradients.)"""
    q, q_mask, d, d_mask = ctx.saved_tensors
    need_q, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[2]          # a frozen encoder's pass is not run
    gq, gd = torch.ops.mm_native.maxsim_inbatch_backward(q, q_mask, d, d_mask, g.contiguous(), ctx.bug_compatible, need_q, need_d)
    return (gq if need_q else None), None, (gd if need_d else None), None, None, None, None


maxsim_inbatch.register_autograd(_maxsim_inbatch_backward, setup_context=_maxsim_inbatch_setup)


def _maxsim_inbatch_autocast(_ks, q, q_mask, d, d_mask, bug_compatible=False, sim_round=False, sum_round=False):
    with torch._C._ExcludeDispatchKeyGuard(_AUTOCAST_KEYS):
        return torch.ops.mm_native.maxsim_inbatch(_ac_cast(q), q_mask, _ac_cast(d), d_mask, bug_compatible, True, False)


_FRAG.impl("maxsim_inbatch", _maxsim_inbatch_autocast, "AutocastCUDA", with_keyset=True)


# ---------------------------------------------------------------------------------------------- kernel pooling
@torch.library.custom_op(_NS + "::kernel_pool", mutates_args=(), device_types="cuda")
def kernel_pool(q: Tensor, d: Tensor, q_mask: Optional[Tensor], d_mask: Optional[Tensor], mu: Tensor, sigma: Tensor,
                alpha: Tensor, w: Tensor, pairs_per_query: int = 1, d_gate: Optional[Tensor] = None,
                clamp_min: float = 1e-10) -> Tensor:
    return ops.kernel_pool(q, d, q_mask, d_mask, mu, sigma, alpha, w, pairs_per_query=pairs_per_query,
                           d_gate=d_gate, clamp_min=clamp_min)


@kernel_pool.register_fake
def _(q, d, q_mask, d_mask, mu, sigma, alpha, w, pairs_per_query=1, d_gate=None, clamp_min=1e-10):
    return q.new_empty((d.shape[0],), dtype=torch.float32)


def _kp_setup(ctx, inputs, output):
    q, d, q_mask, d_mask, mu, sigma, alpha, w, ppq, d_gate, clamp_min = inputs
    ctx.save_for_backward(q, d, q_mask, d_mask, mu, sigma, alpha, w, d_gate)
    ctx.ppq, ctx.clamp_min = ppq, clamp_min


def _kp_backward(ctx, g):
    q, d, q_mask, d_mask, mu, sigma, alpha, w, d_gate = ctx.saved_tensors
    if ctx.ppq != 1:
        raise ops.NativeError("mm_native::kernel_pool backward needs the pair-per-row layout (pairs_per_query = 1)")
    r = ops.kernel_pool_bwd(q, d, q_mask, d_mask, mu, sigma, alpha, w, g, d_gate=d_gate, clamp_min=ctx.clamp_min)
    gg = r[4].view_as(d_gate) if d_gate is not None else None
    return r[0], r[1], None, None, None, None, r[2].view_as(alpha), r[3].view_as(w), None, gg, None


kernel_pool.register_autograd(_kp_backward, setup_context=_kp_setup)
torch.library.register_autocast(_NS + "::kernel_pool", "cuda", torch.float32)


# ---------------------------------------------------------------------------------------------- TKL
@torch.library.custom_op(_NS + "::tkl_window_pool", mutates_args=(), device_types="cuda")
def tkl_window_pool(q_ctx: Tensor, chunks: Tensor, chunk_mask: Tensor, chunk_slot: Tensor, q_mask: Tensor,
                    params: Tensor, B: int, C: int, K: int, saturation: str) -> Tuple[Tensor, Tensor]:
    score, win = ops.tkl_score(q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params, B, C, K, saturation,
                               return_windows=True)
    return score, win


@tkl_window_pool.register_fake
def _(q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params, B, C, K, saturation):
    W = (max(C * 40, 30) - 30) // 2 + 1
    return q_ctx.new_empty((B,), dtype=torch.float32), q_ctx.new_empty((B, W), dtype=torch.float32)


def _tkl_setup(ctx, inputs, output):
    q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params, B, C, K, saturation = inputs
    ctx.save_for_backward(q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params, output[1])
    ctx.meta = (B, C, K, saturation)


def _tkl_backward(ctx, g, _gwin):
    """mm_tkl_bwd: gradients w.r.t. the contextualised query, the contextualised chunks and the packed parameter vector
    (the window scores are an auxiliary output: no gradient flows through them)."""
    q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params, win = ctx.saved_tensors
    B, C, K, saturation = ctx.meta
    gq, gc, gp = ops.tkl_bwd(q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params, win, g, B, C, K, saturation)
    return gq.to(q_ctx.dtype), gc.to(chunks.dtype), None, None, None, gp.view_as(params).to(params.dtype), None, None, None, None


tkl_window_pool.register_autograd(_tkl_backward, setup_context=_tkl_setup)
torch.library.register_autocast(_NS + "::tkl_window_pool", "cuda", torch.float32)


# ---------------------------------------------------------------------------------------------- PACRR
def _pacrr_bwd_fake(q, d, weights):
    """Fake outputs of pacrr_kmax_backward and co_pacrr_kmax_backward: float32 gradients shaped like q, d, the weights, [C]."""
    return (q.new_empty(q.shape, dtype=torch.float32), d.new_empty(d.shape, dtype=torch.float32),
            [w.new_empty(w.shape, dtype=torch.float32) for w in weights],
            [w.new_empty((w.shape[0],), dtype=torch.float32) for w in weights])


def _pacrr_grads(q, d, weights, bshapes, gq, gd, gw, gb):
    """The native float32 gradients in the dtypes and bias shapes of the inputs."""
    return (gq.to(q.dtype), gd.to(d.dtype), [t.to(w.dtype) for t, w in zip(gw, weights)],
            [t.view(s) for t, s in zip(gb, bshapes)])


@torch.library.custom_op(_NS + "::pacrr_kmax", mutates_args=(), device_types="cuda")
def pacrr_kmax(q: Tensor, d: Tensor, weights: List[Tensor], biases: List[Tensor], k: int,
               pairs_per_query: int) -> Tuple[Tensor, Tensor]:
    """(pairs_per_query has no default: the autograd wrapper drops trailing arguments left at their defaults from the input
    structure the backward must return.)  per_query_results [n_pairs, Q, k N] of PACRR (pacrr.py:78-97) and the int32 positions [n_pairs, Q, k N]
    (column | channel << 16) the backward routes through; no gradient flows through the positions."""
    out, idx = ops.pacrr_kmax(q, d, weights, biases, k, pairs_per_query=pairs_per_query, save=True)
    return out, idx


@pacrr_kmax.register_fake
def _(q, d, weights, biases, k, pairs_per_query):
    shape = (d.shape[0], q.shape[1], k * (len(weights) + 1))
    return q.new_empty(shape, dtype=torch.float32), q.new_empty(shape, dtype=torch.int32)


@torch.library.custom_op(_NS + "::pacrr_kmax_backward", mutates_args=(), device_types="cuda")
def pacrr_kmax_backward(q: Tensor, d: Tensor, weights: List[Tensor], idx: Tensor, grad_out: Tensor, k: int,
                        pairs_per_query: int = 1) -> Tuple[Tensor, Tensor, List[Tensor], List[Tensor]]:
    gq, gd, gw, gb = ops.pacrr_kmax_bwd(q, d, weights, idx, grad_out, k, pairs_per_query=pairs_per_query)
    return gq, gd, gw, gb


@pacrr_kmax_backward.register_fake
def _(q, d, weights, idx, grad_out, k, pairs_per_query=1):
    return _pacrr_bwd_fake(q, d, weights)


def _pacrr_setup(ctx, inputs, output):
    q, d, weights, biases, k, ppq = inputs
    ctx.save_for_backward(q, d, output[1], *weights)
    ctx.meta = (k, ppq, [b.shape for b in biases])
    ctx.mark_non_differentiable(output[1])


def _pacrr_backward(ctx, g, _gidx):
    q, d, idx, *weights = ctx.saved_tensors
    k, ppq, bshapes = ctx.meta
    gq, gd, gw, gb = torch.ops.mm_native.pacrr_kmax_backward(q, d, weights, idx, g.contiguous(), k, ppq)
    return _pacrr_grads(q, d, weights, bshapes, gq, gd, gw, gb) + (None, None)


pacrr_kmax.register_autograd(_pacrr_backward, setup_context=_pacrr_setup)
torch.library.register_autocast(_NS + "::pacrr_kmax", "cuda", torch.float32)


# ---------------------------------------------------------------------------------------------- CO-PACRR
@torch.library.custom_op(_NS + "::co_pacrr_kmax", mutates_args=(), device_types="cuda")
def co_pacrr_kmax(q: Tensor, d: Tensor, weights: List[Tensor], biases: List[Tensor], k: int, views: List[int],
                  pairs_per_query: int) -> Tuple[Tensor, Tensor]:
    """per_query_results [n_pairs, Q, 8 k N] of CO-PACRR (co_pacrr.py:90-158) and the int32 positions [n_pairs, Q, N, 4 k]
    (column | channel << 16) the backward routes through; no gradient flows through the positions.  (pairs_per_query has
    no default, as in pacrr_kmax.)"""
    out, idx = ops.co_pacrr_kmax(q, d, weights, biases, k, views, pairs_per_query=pairs_per_query, save=True)
    return out, idx


@co_pacrr_kmax.register_fake
def _(q, d, weights, biases, k, views, pairs_per_query):
    N = len(weights) + 1
    return (q.new_empty((d.shape[0], q.shape[1], 8 * k * N), dtype=torch.float32),
            q.new_empty((d.shape[0], q.shape[1], N, 4 * k), dtype=torch.int32))


@torch.library.custom_op(_NS + "::co_pacrr_kmax_backward", mutates_args=(), device_types="cuda")
def co_pacrr_kmax_backward(q: Tensor, d: Tensor, weights: List[Tensor], idx: Tensor, grad_out: Tensor, k: int,
                           views: List[int], pairs_per_query: int = 1) -> Tuple[Tensor, Tensor, List[Tensor], List[Tensor]]:
    gq, gd, gw, gb = ops.co_pacrr_kmax_bwd(q, d, weights, idx, grad_out, k, views, pairs_per_query=pairs_per_query)
    return gq, gd, gw, gb


@co_pacrr_kmax_backward.register_fake
def _(q, d, weights, idx, grad_out, k, views, pairs_per_query=1):
    return _pacrr_bwd_fake(q, d, weights)


def _co_pacrr_setup(ctx, inputs, output):
    q, d, weights, biases, k, views, ppq = inputs
    ctx.save_for_backward(q, d, output[1], *weights)
    ctx.meta = (k, list(views), ppq, [b.shape for b in biases])
    ctx.mark_non_differentiable(output[1])


def _co_pacrr_backward(ctx, g, _gidx):
    q, d, idx, *weights = ctx.saved_tensors
    k, views, ppq, bshapes = ctx.meta
    gq, gd, gw, gb = torch.ops.mm_native.co_pacrr_kmax_backward(q, d, weights, idx, g.contiguous(), k, views, ppq)
    return _pacrr_grads(q, d, weights, bshapes, gq, gd, gw, gb) + (None, None, None)


co_pacrr_kmax.register_autograd(_co_pacrr_backward, setup_context=_co_pacrr_setup)
torch.library.register_autocast(_NS + "::co_pacrr_kmax", "cuda", torch.float32)


# ---------------------------------------------------------------------------------------------- DRMM
@torch.library.custom_op(_NS + "::drmm_hist", mutates_args=(), device_types="cuda")
def drmm_hist(q: Tensor, d: Tensor, bins: int = 10, pairs_per_query: int = 1, d_len: Optional[Tensor] = None,
              clamp: bool = False) -> Tensor:
    """hist [n_pairs, Q, bins] of DRMM (drmm.py:66-74).  Piecewise constant in q and d: no gradient flows through it."""
    return ops.drmm_hist(q, d, bins, pairs_per_query, d_len, clamp)


@drmm_hist.register_fake
def _(q, d, bins=10, pairs_per_query=1, d_len=None, clamp=False):
    return q.new_empty((d.shape[0], q.shape[1], bins), dtype=torch.float32)


def _drmm_hist_setup(ctx, inputs, output):
    ctx.mark_non_differentiable(output)


def _drmm_hist_backward(ctx, g):
    return None, None, None, None, None, None


drmm_hist.register_autograd(_drmm_hist_backward, setup_context=_drmm_hist_setup)
torch.library.register_autocast(_NS + "::drmm_hist", "cuda", torch.float32)


@torch.library.custom_op(_NS + "::drmm_score", mutates_args=(), device_types="cuda")
def drmm_score(q: Tensor, d: Tensor, gate: Tensor, W1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
               pairs_per_query: int = 1, d_len: Optional[Tensor] = None, clamp: bool = False) -> Tensor:
    """score [n_pairs] of DRMM with the head fused (inference only: no autograd formula is registered, so a call whose
    inputs require grad raises; train through drmm_hist + the torch head)."""
    return ops.drmm_score(q, d, gate, W1, b1, w2, b2, pairs_per_query, d_len, clamp)


@drmm_score.register_fake
def _(q, d, gate, W1, b1, w2, b2, pairs_per_query=1, d_len=None, clamp=False):
    return q.new_empty((d.shape[0],), dtype=torch.float32)


def _drmm_score_setup(ctx, inputs, output):
    pass


def _drmm_score_backward(ctx, g):
    raise ops.NativeError("mm_native::drmm_score is inference-only (the head is fused into the histogram kernel); "
                          "for training call mm_native::drmm_hist and apply the head in torch")


drmm_score.register_autograd(_drmm_score_backward, setup_context=_drmm_score_setup)
torch.library.register_autocast(_NS + "::drmm_score", "cuda", torch.float32)


# ---------------------------------------------------------------------------------------------- MatchPyramid
@torch.library.custom_op(_NS + "::matchpyramid_features", mutates_args=(), device_types="cuda")
def matchpyramid_features(q: Tensor, d: Tensor, weights: List[Tensor], biases: List[Tensor], pool_sizes: List[int],
                          pairs_per_query: int = 1) -> Tensor:
    """features [n_pairs, C_L ph_L pw_L] of MatchPyramid (matchpyramid.py:74-92); pool_sizes is flat: ph_0, pw_0, ph_1, ...
    Inference only: no autograd formula exists, so a backward through it raises; train through the module's torch layers."""
    pools = [(pool_sizes[2 * i], pool_sizes[2 * i + 1]) for i in range(len(pool_sizes) // 2)]
    return ops.matchpyramid_features(q, d, weights, biases, pools, pairs_per_query)


@matchpyramid_features.register_fake
def _(q, d, weights, biases, pool_sizes, pairs_per_query=1):
    return q.new_empty((d.shape[0], weights[-1].shape[0] * pool_sizes[-2] * pool_sizes[-1]), dtype=torch.float32)


def _matchpyramid_setup(ctx, inputs, output):
    pass


def _matchpyramid_backward(ctx, g):
    raise ops.NativeError("mm_native::matchpyramid_features is inference-only (forward kernel only); for training run the "
                          "module's own torch layers (matchmaker_amd.matchpyramid.MatchPyramid does so when anything "
                          "requires a gradient)")


matchpyramid_features.register_autograd(_matchpyramid_backward, setup_context=_matchpyramid_setup)
torch.library.register_autocast(_NS + "::matchpyramid_features", "cuda", torch.float32)


def _mp_pools(pool_sizes):
    return [(pool_sizes[2 * i], pool_sizes[2 * i + 1]) for i in range(len(pool_sizes) // 2)]


@torch.library.custom_op(_NS + "::matchpyramid_features_train", mutates_args=(), device_types="cuda")
def matchpyramid_features_train(q: Tensor, d: Tensor, weights: List[Tensor], biases: List[Tensor], pool_sizes: List[int],
                                pairs_per_query: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(features, pooled, argmax): matchpyramid_features (the same bits) with the state its backward routes through
    (ops.matchpyramid_features_save): pooled [n_pairs, S] float32 and argmax [n_pairs, S] int32, S = sum_l C_l ph_l pw_l.
    Differentiable in q, d, weights and biases through `features` only; no gradient flows through the saved state.
    (pairs_per_query has no default, as in pacrr_kmax.)"""
    out, (pooled, argmax) = ops.matchpyramid_features_save(q, d, weights, biases, _mp_pools(pool_sizes), pairs_per_query)
    return out, pooled, argmax


@matchpyramid_features_train.register_fake
def _(q, d, weights, biases, pool_sizes, pairs_per_query):
    B = d.shape[0]
    S = sum(w.shape[0] * pool_sizes[2 * i] * pool_sizes[2 * i + 1] for i, w in enumerate(weights))
    return (q.new_empty((B, weights[-1].shape[0] * pool_sizes[-2] * pool_sizes[-1]), dtype=torch.float32),
            q.new_empty((B, S), dtype=torch.float32), q.new_empty((B, S), dtype=torch.int32))


@torch.library.custom_op(_NS + "::matchpyramid_features_train_backward", mutates_args=(), device_types="cuda")
def matchpyramid_features_train_backward(q: Tensor, d: Tensor, weights: List[Tensor], biases: List[Tensor],
                                         pool_sizes: List[int], pooled: Tensor, argmax: Tensor, grad_out: Tensor,
                                         pairs_per_query: int = 1) -> Tuple[Tensor, Tensor, List[Tensor], List[Tensor]]:
    """No autograd formula: a double backward raises."""
    gq, gd, gw, gb = ops.matchpyramid_bwd(q, d, weights, biases, _mp_pools(pool_sizes), (pooled, argmax), grad_out,
                                          pairs_per_query)
    return gq, gd, gw, gb


@matchpyramid_features_train_backward.register_fake
def _(q, d, weights, biases, pool_sizes, pooled, argmax, grad_out, pairs_per_query=1):
    return (q.new_empty(q.shape, dtype=torch.float32), d.new_empty(d.shape, dtype=torch.float32),
            [w.new_empty(w.shape, dtype=torch.float32) for w in weights],
            [b.new_empty(b.shape, dtype=torch.float32) for b in biases])


def _matchpyramid_train_setup(ctx, inputs, output):
    q, d, weights, biases, pool_sizes, ppq = inputs
    ctx.save_for_backward(q, d, output[1], output[2], *weights, *biases)
    ctx.meta = (list(pool_sizes), ppq, len(weights))
    ctx.mark_non_differentiable(output[1], output[2])


def _matchpyramid_train_backward(ctx, g, _gpooled, _gargmax):
    q, d, pooled, argmax, *params = ctx.saved_tensors
    pool_sizes, ppq, L = ctx.meta
    weights, biases = params[:L], params[L:]
    gq, gd, gw, gb = torch.ops.mm_native.matchpyramid_features_train_backward(q, d, weights, biases, pool_sizes, pooled,
                                                                              argmax, g.contiguous(), ppq)
    return (gq.to(q.dtype), gd.to(d.dtype), [t.to(w.dtype) for t, w in zip(gw, weights)],
            [t.to(b.dtype) for t, b in zip(gb, biases)], None, None)


matchpyramid_features_train.register_autograd(_matchpyramid_train_backward, setup_context=_matchpyramid_train_setup)
torch.library.register_autocast(_NS + "::matchpyramid_features_train", "cuda", torch.float32)


# ---------------------------------------------------------------------------------------------- ColBERT retrieval
@torch.library.custom_op(_NS + "::colbert_candidates", mutates_args=(), device_types="cuda")
def colbert_candidates(hit_rows: Tensor, begin_sorted: Tensor, end_sorted: Tensor, doc_of_sorted: Tensor, T: int,
                       c_cap: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(cand_doc [nq, c_cap] int32, cand_begin, cand_end [nq, c_cap] int64, count [nq] int32): the documents that own the token
    hits of every query (dense_retrieval.py:391-412).  Integer in, integer out: no autograd formula."""
    return ops.colbert_candidates(hit_rows, begin_sorted, end_sorted, doc_of_sorted, T, c_cap)


@colbert_candidates.register_fake
def _(hit_rows, begin_sorted, end_sorted, doc_of_sorted, T, c_cap=None):
    nq, H = hit_rows.shape
    C = min(H, begin_sorted.shape[0]) if c_cap is None else c_cap
    return (hit_rows.new_empty((nq, C), dtype=torch.int32), hit_rows.new_empty((nq, C), dtype=torch.int64),
            hit_rows.new_empty((nq, C), dtype=torch.int64), hit_rows.new_empty((nq,), dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- MaxP retrieval
@torch.library.custom_op(_NS + "::distinct_hits", mutates_args=(), device_types="cuda")
def distinct_hits(scores: Tensor, ids: Tensor, top_n: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(scores [nq, top_n] float32, ids [nq, top_n] int64, pos [nq, top_n] int32, n_distinct [nq] int32, n_valid [nq] int32): the
    first hit of every document in a query's passage hits (ops.distinct_hits; dense_retrieval.py:414-429).  A selection: no
    autograd formula."""
    return ops.distinct_hits(scores, ids, top_n)


@distinct_hits.register_fake
def _(scores, ids, top_n):
    nq = scores.shape[0]
    return (scores.new_empty((nq, top_n), dtype=torch.float32), scores.new_empty((nq, top_n), dtype=torch.int64),
            scores.new_empty((nq, top_n), dtype=torch.int32), scores.new_empty((nq,), dtype=torch.int32),
            scores.new_empty((nq,), dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- fp8 token store
@torch.library.custom_op(_NS + "::fp8_quantize_rows", mutates_args=(), device_types="cuda")
def fp8_quantize_rows(x: Tensor) -> Tuple[Tensor, Tensor]:
    """(codes [T, E] uint8 = OCP e4m3fn bytes, scales [T] float32 powers of two) of token rows x [T, E] (ops.fp8_quantize_rows).
    A rounding, not a differentiable function: no autograd formula."""
    return ops.fp8_quantize_rows(x)


@fp8_quantize_rows.register_fake
def _(x):
    T, E = x.shape
    return x.new_empty((T, E), dtype=torch.uint8), x.new_empty((T,), dtype=torch.float32)


@torch.library.custom_op(_NS + "::maxsim_ragged_fp8", mutates_args=(), device_types="cuda")
def maxsim_ragged_fp8(q: Tensor, codes: Tensor, scales: Tensor, doc_begin: Tensor, doc_end: Tensor,
                      q_mask: Optional[Tensor] = None, pairs_per_query: int = 1, check_ranges: bool = True,
                      sim_round: bool = False, sum_round: bool = False) -> Tensor:
    """[n_pairs] float32: the ragged MaxSim over an fp8 token store (ops.maxsim_ragged_fp8).  Forward only, like
    colbert_candidates: a retrieval-time operator over a frozen store."""
    return ops.maxsim_ragged_fp8(q, codes, scales, doc_begin, doc_end, q_mask, pairs_per_query=pairs_per_query,
                                 check_ranges=check_ranges, sim_round=sim_round, sum_round=sum_round)


@maxsim_ragged_fp8.register_fake
def _(q, codes, scales, doc_begin, doc_end, q_mask=None, pairs_per_query=1, check_ranges=True, sim_round=False,
      sum_round=False):
    return q.new_empty((doc_begin.numel(),), dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- graph index
@torch.library.custom_op(_NS + "::graph_search", mutates_args=(), device_types="cuda")
def graph_search(queries: Tensor, vectors: Tensor, neighbors: Tensor, entry_rows: Tensor, ef: int, k: int, width: int = 4,
                 max_iters: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(scores [nq, k] float32, rows [nq, k] int64, stats [nq, 2] int32 = (iterations run, rows scored)): the beam search of
    the graph index (ops.graph_search).  A search, not a differentiable function: no autograd formula."""
    s, r, st = ops.graph_search(queries, vectors, neighbors, entry_rows, ef, k, width, max_iters, return_stats=True)
    return s, r, st


@graph_search.register_fake
def _(queries, vectors, neighbors, entry_rows, ef, k, width=4, max_iters=None):
    nq = queries.shape[0]
    return (queries.new_empty((nq, k), dtype=torch.float32), queries.new_empty((nq, k), dtype=torch.int64),
            queries.new_empty((nq, 2), dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- ranking
@torch.library.custom_op(_NS + "::segment_rank", mutates_args=(), device_types="cuda")
def segment_rank(scores: Tensor, seg_begin: Tensor, max_len: int) -> Tensor:
    """order [N] int32: per-query rank order of flat scores (ops.segment_rank; utils/core_metrics.py:502-511).  A
    permutation, not a differentiable function: no autograd formula."""
    return ops.segment_rank(scores, seg_begin, max_len)


@segment_rank.register_fake
def _(scores, seg_begin, max_len):
    return scores.new_empty((scores.shape[0],), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------- training losses
from . import losses as _losses  # noqa: E402


@torch.library.custom_op(_NS + "::pair_loss", mutates_args=(), device_types="cuda")
def pair_loss(pos: Tensor, neg: Tensor, a: Tensor, b: Optional[Tensor], kind: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(loss [] float32, grad_pos, grad_neg): a pairwise / pointwise training loss with its gradient (losses.pair_loss;
    kind = a value of losses.PAIR_KINDS).  Differentiable in pos and neg through `loss`; the labels get no gradient."""
    return _losses.pair_loss(pos, neg, a, b, kind)


@pair_loss.register_fake
def _(pos, neg, a, b, kind):
    return pos.new_empty((), dtype=torch.float32), pos.new_empty(pos.shape), neg.new_empty(pos.shape)


def _pair_loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1], output[2])
    ctx.mark_non_differentiable(output[1], output[2])


def _pair_loss_backward(ctx, g, _gpos, _gneg):
    gpos, gneg = ctx.saved_tensors
    return gpos * g, gneg * g, None, None, None


pair_loss.register_autograd(_pair_loss_backward, setup_context=_pair_loss_setup)


@torch.library.custom_op(_NS + "::list_loss", mutates_args=(), device_types="cuda")
def list_loss(scores: Tensor, labels: Tensor, kind: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(loss [] float32, per_list [B] float32, grad [B, L]): a listwise training loss with its gradient (losses.list_loss;
    kind = a value of losses.LIST_KINDS).  Differentiable in scores through `loss` and `per_list`; the labels get no gradient."""
    return _losses.list_loss(scores, labels, kind)


@list_loss.register_fake
def _(scores, labels, kind):
    return (scores.new_empty((), dtype=torch.float32), scores.new_empty((scores.shape[0],), dtype=torch.float32),
            scores.new_empty(scores.shape))


def _list_loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2])
    ctx.kind = inputs[2]
    ctx.mark_non_differentiable(output[2])


def _list_loss_backward(ctx, g_loss, g_per_list, _ggrad):
    return _losses.list_loss_backward(ctx.saved_tensors[0], ctx.kind, g_loss, g_per_list), None, None


list_loss.register_autograd(_list_loss_backward, setup_context=_list_loss_setup)


# ---------------------------------------------------------------------------------------------- in-batch negatives
from . import inbatch as _inbatch  # noqa: E402


@torch.library.custom_op(_NS + "::inbatch_dot_loss", mutates_args=(), device_types="cuda")
def inbatch_dot_loss(q: Tensor, dp: Tensor, dn: Tensor, sp: Tensor, tp: Optional[Tensor], tn: Optional[Tensor], family: int,
                     kind: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(loss [], stats [3], grad_q, grad_dp, grad_dn, grad_sp): the in-batch negatives of train.py:434-472 from the vectors
    (inbatch.inbatch_dot_loss; family = inbatch.FAMILIES value, kind = a value of losses.PAIR_KINDS / LIST_KINDS).
    Differentiable in q, dp, dn and sp through `loss`; the teacher matrices get no gradient."""
    return _inbatch.inbatch_dot_loss(q, dp, dn, sp, tp, tn, family, kind)


@inbatch_dot_loss.register_fake
def _(q, dp, dn, sp, tp, tn, family, kind):
    return (q.new_empty((), dtype=torch.float32), q.new_empty((3,), dtype=torch.float32), q.new_empty(q.shape), dp.new_empty(q.shape),
            dn.new_empty(q.shape), sp.new_empty(sp.shape))


def _inbatch_dot_setup(ctx, inputs, output):
    ctx.save_for_backward(*output[2:])
    ctx.mark_non_differentiable(*output[1:])


def _inbatch_dot_backward(ctx, g, *_unused):
    return tuple(_inbatch._scaled(t, g, True) for t in ctx.saved_tensors) + (None,) * 4


inbatch_dot_loss.register_autograd(_inbatch_dot_backward, setup_context=_inbatch_dot_setup)


@torch.library.custom_op(_NS + "::inbatch_select_loss", mutates_args=(), device_types="cuda")
def inbatch_select_loss(sp: Tensor, s_pos: Tensor, s_neg: Tensor, tp: Optional[Tensor], tn: Optional[Tensor], family: int,
                        kind: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(loss [], stats [3], grad_sp, grad_s_pos, grad_s_neg): the in-batch negatives over [B, B] score matrices
    (inbatch.inbatch_select_loss).  Differentiable in sp, s_pos and s_neg through `loss`."""
    return _inbatch.inbatch_select_loss(sp, s_pos, s_neg, tp, tn, family, kind)


@inbatch_select_loss.register_fake
def _(sp, s_pos, s_neg, tp, tn, family, kind):
    return (sp.new_empty((), dtype=torch.float32), sp.new_empty((3,), dtype=torch.float32), sp.new_empty(sp.shape),
            s_pos.new_empty(s_pos.shape), s_neg.new_empty(s_pos.shape))


def _inbatch_select_setup(ctx, inputs, output):
    ctx.save_for_backward(*output[2:])
    ctx.mark_non_differentiable(*output[1:])


def _inbatch_select_backward(ctx, g, *_unused):
    return tuple(_inbatch._scaled(t, g, True) for t in ctx.saved_tensors) + (None,) * 4


inbatch_select_loss.register_autograd(_inbatch_select_backward, setup_context=_inbatch_select_setup)


# ---------------------------------------------------------------------------------------------- contextualiser attention
from . import contextualize as _contextualize  # noqa: E402


@torch.library.custom_op(_NS + "::self_attention", mutates_args=(), device_types="cuda")
def self_attention(qkv: Tensor, mask: Optional[Tensor], num_heads: int) -> Tensor:
    """out [B, L, E] of qkv's dtype: the attention core of the TK-family contextualiser on the in-projection qkv [B, L, 3E]
    with a key mask (contextualize.self_attention).  No autograd formula: the operator serves inference."""
    return _contextualize.self_attention(qkv, mask, num_heads)


@self_attention.register_fake
def _(qkv, mask, num_heads):
    return qkv.new_empty((qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3))
