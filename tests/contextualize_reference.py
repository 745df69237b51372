"""float64 restatement of the TK-family contextualiser (a helper, not a test module): the attention core with the safe softmax
(a sequence with no unmasked key gives 0, as torch 2.10's math path does) and the post-norm nn.TransformerEncoder layer stack
around it, from a module's own parameters.  Also the mask patterns, the tolerances and the data of the contextualiser tests.

Tolerance rule: a result is within 4 x the error of a reference fp32 evaluation of the same inputs
against float64, plus 4 fp32 ulps of the float64 value; the factor 4 is the project's margin for another accumulation order."""
import functools
import math

import numpy as np
import torch

PATTERNS = ("full", "prefix", "front", "holes", "none")


def ulp32(x):
    """the fp32 ulp at |x| (elementwise, float64)"""
    mag = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(mag)) - 23)


def mask_pattern(name, L):
    """one {0,1} row of L positions: every token, a prefix, 5 leading zeros (as many as leave a token), interior holes, nothing"""
    m = np.ones(L, dtype=np.float32)
    if name == "prefix":
        m[max(1, (2 * L) // 3):] = 0
    elif name == "front":
        m[:min(5, L - 1)] = 0
    elif name == "holes":
        m[1::3] = 0
        if L > 4:
            m[L // 2:L // 2 + 2] = 0
    elif name == "none":
        m[:] = 0
    else:
        assert name == "full", name
    return m


def masks(L, patterns=PATTERNS):
    return np.stack([mask_pattern(p, L) for p in patterns])


def attention64(qkv, mask, H):
    """out [B, L, E] float64 of qkv [B, L, 3E] (Q | K | V, head h at column h dh) under the key mask [B, L] (nonzero = token)"""
    qkv = np.asarray(qkv, dtype=np.float64)
    B, L, E3 = qkv.shape
    E = E3 // 3
    dh = E // H
    q, k, v = (qkv[:, :, i * E:(i + 1) * E].reshape(B, L, H, dh) for i in range(3))
    s = np.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(dh)
    keep = np.asarray(mask) != 0
    s = np.where(keep[:, None, None, :], s, -np.inf)
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    w = np.where(l > 0, p / np.where(l > 0, l, 1.0), 0.0)
    return np.einsum("bhij,bjhd->bihd", w, v).reshape(B, L, E)


def sdpa32(qkv, mask, H):
    """torch's own fp32 evaluation on the CPU: scaled_dot_product_attention with the boolean mask -> float64 [B, L, E]"""
    t = torch.from_numpy(np.array(qkv, dtype=np.float32))
    B, L, E3 = t.shape
    E = E3 // 3
    q, k, v = (t[:, :, i * E:(i + 1) * E].reshape(B, L, H, E // H).transpose(1, 2) for i in range(3))
    keep = torch.as_tensor(np.asarray(mask) != 0)[:, None, None, :].expand(B, 1, L, L)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=keep)
    return o.transpose(1, 2).reshape(B, L, E).double().numpy()


def live_rows(mask):
    """[B] bool: sequences with at least one unmasked key"""
    return (np.asarray(mask) != 0).any(axis=1)


def attention_bound(qkv, mask, H, ref64=None):
    """(ref64, bound, e_ref): |got - ref64| <= 4 e_ref + 4 ulp32(|ref64|), e_ref = the largest error of torch's fp32 evaluation
    of the same inputs, the sequences with no unmasked key left out of it (the tests ask exactly +0 of those)"""
    ref64 = attention64(qkv, mask, H) if ref64 is None else ref64
    live = live_rows(mask)
    e_ref = float(np.abs(sdpa32(qkv, mask, H)[live] - ref64[live]).max()) if live.any() else 0.0
    return ref64, 4 * e_ref + 4 * ulp32(ref64), e_ref


@functools.lru_cache(maxsize=None)
def random_qkv(L, H, dh, scale, B=5, seed=0):
    """N(0,1) data [B, L, 3 H dh] float32 with q and k at `scale`, and the five mask patterns"""
    rng = np.random.default_rng([seed, L, H, dh, int(scale)])
    E = H * dh
    x = rng.standard_normal((B, L, 3 * E))
    x[:, :, :2 * E] *= scale
    x = x.astype(np.float32)
    x.setflags(write=False)
    m = masks(L, PATTERNS[:B] if B <= len(PATTERNS) else PATTERNS)
    m.setflags(write=False)
    return x, m


# ---- the layer stack -----------------------------------------------------------------------------------------------------------
def _ln(x, norm):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), norm.weight.double(), norm.bias.double(), norm.eps)


def encoder64(encoder, x, mask):
    """nn.TransformerEncoder (post-norm layers, ReLU or GELU, no dropout) on batch-first x [B, L, E] with sequence_mask
    [B, L] (1 = token) in float64, from the (CPU) module's own parameters -> float64 numpy [B, L, E]"""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    with torch.no_grad():
        for layer in encoder.layers:
            assert not layer.norm_first
            att = layer.self_attn
            qkv = x @ att.in_proj_weight.double().t() + att.in_proj_bias.double()
            a = torch.as_tensor(attention64(qkv.numpy(), mask, att.num_heads))
            a = a @ att.out_proj.weight.double().t() + att.out_proj.bias.double()
            x = _ln(x + a, layer.norm1)
            h = x @ layer.linear1.weight.double().t() + layer.linear1.bias.double()
            act = layer.activation
            h = torch.nn.functional.gelu(h) if (act is torch.nn.functional.gelu or isinstance(act, torch.nn.GELU)) else torch.relu(h)
            x = _ln(x + h @ layer.linear2.weight.double().t() + layer.linear2.bias.double(), layer.norm2)
        if encoder.norm is not None:
            x = _ln(x, encoder.norm)
    return x.numpy()


def tk_representation64(model, emb, mask, pos):
    """ECAI20_TK.forward_representation (ecai20_tk.py:133-143) in float64 from a CPU module's parameters"""
    emb = np.asarray(emb, dtype=np.float64)
    ctx = encoder64(model.contextualizer, emb + np.asarray(pos, dtype=np.float64), mask)
    if not model.mix_hybrid_context:
        return ctx
    mix = float(model.mixer.detach().double())
    return mix * emb + (1 - mix) * ctx


def golden_tol(ref, E):
    """4 fp32 ulps of the largest magnitude x sqrt(E): the error of an fp32 evaluation whose reductions run over E terms"""
    return 4 * float(ulp32(np.abs(ref).max())) * math.sqrt(E)
