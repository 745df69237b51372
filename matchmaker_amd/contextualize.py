"""The contextualiser of the TK family (ECAI20_TK, TKL_sigir20, CIKM20_TK_Sparse, IDCM's sampler) with its attention core on
libmm_native.so (csrc/self_attention.hip):

    self_attention(qkv, mask, num_heads)            -> out [B, L, E]      mm_self_attention_fwd
    encode(encoder, x, sequence_mask, native)       -> ctx [B, L, E]      the models' nn.TransformerEncoder call
    enable(model, on=True)                          sets `native_attention` on every module that has it

The reference builds its encoders with batch_first=False and passes a key-padding mask (ecai20_tk.py:57-58, :138;
sigir20_tkl.py:296-308; sigir21_idcm.py:96-97, :174-175), so every layer runs F.multi_head_attention_forward and
scaled_dot_product_attention with a materialised float mask.  `encode(native=True)` runs the same layers batch-first from the same
parameters: F.linear in-projection, the fused attention kernel on the [B, L, 3E] projection as it lies in memory, out_proj,
norm1, the feed-forward block, norm2.  The projections, LayerNorm and the feed-forward block stay torch's; there is no backward:
a call that needs a gradient, a CPU tensor, a layer the route does not know or a shape outside the kernel's envelope runs
exactly the statement the models had, and training is unchanged.  A call that takes the native route and fails raises: nothing
falls back after the decision.

The torch <-> ABI wrapper lives here, not in ops.py (ops.self_attention forwards); the module has its own `torch`, `_workspace`
and `clear_workspaces` names and allocates its output with `torch.empty`, so tests/poison.py can be pointed at it.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import NativeError
from .ops import _DT, _call, _dev_check, _mask, _workspace, clear_workspaces  # noqa: F401  (re-exported: tests/poison.py patches them here)


def supported(dtype, L: int, H: int, dh: int) -> bool:
    """mm_self_attention_supported: whether the kernel takes sequences of L tokens with H heads of dh columns in `dtype`
    (1 <= L <= 256, 1 <= dh <= 64, dh even for float16 / bfloat16)."""
    if dtype not in _DT:
        return False
    return bool(_lib.lib().mm_self_attention_supported(_DT[dtype], int(L), int(H), int(dh)))


# ---- torch <-> ABI ---------------------------------------------------------------------------------------------------------
def self_attention(qkv, mask, num_heads: int):
    """out [B, L, E] like qkv: softmax(q k^T / sqrt(dh) + key mask) v per head, heads concatenated (native
    mm_self_attention_fwd; the attention core of ecai20_tk.py:138, sigir20_tkl.py:296-308, sigir21_idcm.py:174-175).

    qkv [B, L, 3E] float32 / float16 / bfloat16 as F.linear(x, in_proj_weight, in_proj_bias) returns it (Q | K | V, head h at
    column h * E / num_heads); made contiguous, at any element-aligned address.  mask: None | [B] lengths | [B, L] bool / uint8 /
    int64 / float (nonzero = token), an arbitrary pattern; only keys are masked, every query row is computed, and a sequence with
    no token gets +0.  Accumulation, softmax and normalisation in float32, one rounding at the store.  Raises NativeError for CPU
    tensors, for tensors that require grad (there is no backward) and, with .code == MM_EUNSUPPORTED, for shapes `supported`
    refuses.  One launch on the current stream, no workspace, no read-back: graph-capturable, bit-equal from run to run."""
    op = "self_attention"
    dev = _dev_check(qkv, mask)
    if qkv.requires_grad or (mask is not None and mask.requires_grad):
        raise NativeError(f"{op}: there is no native backward (detach the tensors, or use the encoder's own layers)")
    if qkv.dim() != 3 or qkv.dtype not in _DT or num_heads < 1 or qkv.shape[2] % (3 * num_heads):
        raise NativeError(f"{op}: qkv must be float32 / float16 / bfloat16 [B, L, 3 * num_heads * dh], got {qkv.dtype} "
                          f"{tuple(qkv.shape)} for {num_heads} heads")
    B, L, E3 = qkv.shape
    E = E3 // 3
    dh = E // num_heads
    if not supported(qkv.dtype, L, num_heads, dh):
        raise NativeError(f"{op}: L={L}, {num_heads} heads of {dh} columns in {qkv.dtype} are outside the kernel's envelope "
                          "(1 <= L <= 256, 1 <= dh <= 64, dh even for 16-bit types)", _lib.MM_EUNSUPPORTED)
    qkv = qkv.contiguous()
    mk, mp, kind = _mask(mask, B, L, "mask")
    out = torch.empty((B, L, E), dtype=qkv.dtype, device=dev)
    _call(dev, _lib.lib().mm_self_attention_fwd, (qkv.data_ptr(), _DT[qkv.dtype], mp, kind, B, L, num_heads, dh, out.data_ptr()),
          stream_only=True)
    return out


# ---- the route ----------------------------------------------------------------------------------------------------------------
def _plain(encoder, x, sequence_mask):
    return encoder(x.transpose(1, 0), src_key_padding_mask=~sequence_mask.bool()).transpose(1, 0)


def _act_ok(act):
    return act is F.relu or act is F.gelu or isinstance(act, (nn.ReLU, nn.GELU))


def _layer_ok(layer):
    if not isinstance(layer, nn.TransformerEncoderLayer) or layer.norm_first or not _act_ok(layer.activation):
        return False
    att = layer.self_attn
    if (not isinstance(att, nn.MultiheadAttention) or att.in_proj_weight is None or att.bias_k is not None or att.bias_v is not None
            or att.add_zero_attn or att.embed_dim % att.num_heads):
        return False
    drop = max(layer.dropout.p, layer.dropout1.p, layer.dropout2.p, att.dropout)
    return drop == 0 or not layer.training


def _qkv_dtype(x, weight):
    """the dtype F.linear(x, weight) has in the current autocast state"""
    if torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return torch.promote_types(x.dtype, weight.dtype)


def eligible(encoder, x, sequence_mask) -> bool:
    """whether encode(native=True) takes the native route for these arguments"""
    if not (isinstance(encoder, nn.TransformerEncoder) and isinstance(x, torch.Tensor) and isinstance(sequence_mask, torch.Tensor)):
        return False
    if not (x.is_cuda and sequence_mask.is_cuda and x.device == sequence_mask.device and x.dim() == 3 and x.dtype in _DT
            and tuple(sequence_mask.shape) == tuple(x.shape[:2])):
        return False
    if len(encoder.layers) == 0 or not all(_layer_ok(layer) for layer in encoder.layers):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or sequence_mask.requires_grad or any(p.requires_grad for p in encoder.parameters())):
        return False
    if any(p.device != x.device for p in encoder.parameters()):
        return False
    L, E = x.shape[1], x.shape[2]
    for layer in encoder.layers:
        att = layer.self_attn
        if att.embed_dim != E or not supported(_qkv_dtype(x, att.in_proj_weight), L, att.num_heads, E // att.num_heads):
            return False
    return True


def encode(encoder, x, sequence_mask, native: bool = False):
    """ctx [B, L, E] = encoder(x.transpose(1, 0), src_key_padding_mask=~sequence_mask.bool()).transpose(1, 0) for batch-first
    x [B, L, E] and sequence_mask [B, L] (1 = token).  native=False, or any call that is not `eligible`, runs exactly that
    statement.  An eligible call (HIP tensors, nothing that needs a gradient, post-norm ReLU / GELU layers with dropout 0 or in
    eval mode, a shape the kernel takes) runs the layers batch-first with the fused attention kernel between in_proj and
    out_proj, from the same parameters; under autocast the linears give a 16-bit projection and the 16-bit kernel serves it."""
    if not native or not eligible(encoder, x, sequence_mask):
        return _plain(encoder, x, sequence_mask)
    for layer in encoder.layers:
        att = layer.self_attn
        qkv = F.linear(x, att.in_proj_weight, att.in_proj_bias)
        a = att.out_proj(self_attention(qkv, sequence_mask, att.num_heads))
        x = layer.norm1(x + a)
        x = layer.norm2(x + layer.linear2(layer.activation(layer.linear1(x))))
    if encoder.norm is not None:
        x = encoder.norm(x)
    return x


def enable(model, on: bool = True):
    """Sets `native_attention` on every module of `model` that has the attribute (ECAI20_TK, TKL_sigir20, CIKM20_TK_Sparse);
    returns the number of modules it set.  Nothing else changes: parameters, buffers and state_dict keys stay."""
    n = 0
    for m in model.modules():
        if hasattr(m, "native_attention"):
            m.native_attention = bool(on)
            n += 1
    return n


__all__ = ["self_attention", "supported", "eligible", "encode", "enable"]
