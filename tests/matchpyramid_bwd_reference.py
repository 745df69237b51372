"""Oracles of MatchPyramid's backward (mm_matchpyramid_fwd_save / mm_matchpyramid_bwd), both torch autograd on the CPU, in
fp64 (the yardstick) and in fp32 (what an fp32 evaluation loses):

    (a) the module's own layers: MatchPyramid.torch_features, i.e. nn.AdaptiveMaxPool2d and the .norm-based cosine (not
        tests/matchpyramid_reference.py's amax, whose backward splits the gradient among ties);
    (b) the "given arg-max" form: the same layers with every pooling replaced by relu(conv).flatten(2).gather(-1, argmax):
        the exact gradient for a stated selection.

Also the per-element strict gap (the maximum of a pooling window minus the largest value strictly below it, fp64), which
says where an fp32 arg-max is decided, and the tolerance rule of DESIGN.md §3.9 / §3.11:

    tol = 4 max |g32 - g64| + c 2^-24 max |g64|,  c = max(16, sqrt(n)),  n = the longest sum the kernel forms for the tensor.

Inputs (shared by the CPU and GPU files): g = torch.Generator().manual_seed(5); q = randn(B, Q, E), d = randn(B, D, E),
grad_features = randn(B, F) in that order; conv parameters from MR.random_params(channels, kernels, pools, seed=7, scale=3.0).
Everything here is computed once per case and shared; callers must not modify what they get."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import matchpyramid_reference as MR

# name -> (B, Q, D, E, channels, kernels, pools)
CASES = {
    "tiny": (3, 5, 7, 8, [4, 4], [[3, 3], [3, 3]], [[4, 6], [2, 3]]),              # overlapping windows, exact bias ties
    "rect": (2, 6, 11, 12, [3, 5], [[2, 3], [3, 1]], [[5, 7], [2, 2]]),            # the pad / kernel transposition
    "up": (2, 3, 4, 8, [2, 2], [[3, 3], [1, 1]], [[5, 6], [3, 4]]),                # ph > n: one arg-max of many windows
    "chan": (2, 9, 40, 16, [32, 17], [[3, 3], [5, 5]], [[6, 20], [3, 5]]),         # two channel tiles, K = 800 chains
    "ref": (4, 30, 200, 32, *MR.DEFAULT),                                          # the reference-config instantiation
    "zero": (3, 5, 7, 8, [4, 4], [[3, 3], [3, 3]], [[4, 6], [2, 3]]),              # tiny with zero rows, positive biases
    # beyond the issue's table: code paths none of its cases reaches
    "wide": (2, 6, 40, 8, [3, 2], [[3, 3], [3, 3]], [[3, 2], [2, 1]]),             # a pooling window of 20 conv columns: wider
                                                                                   # than a 16-column tile (the running arg-max)
    "big": (2, 40, 300, 8, [4, 3], [[3, 3], [3, 3]], [[8, 30], [2, 3]]),           # Q > 32: two cosine row tiles, 48-row
                                                                                   # coefficient tiles; D > 256: not FAST
}
DIRECT = ["tiny", "rect", "up"]      # the cases whose fp64 arg-max is separated from fp32 noise (asserted on the CPU)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (q, d, grad_features, params)"""
    B, Q, D, E, channels, kernels, pools = CASES[name]
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    feat = channels[-1] * pools[-1][0] * pools[-1][1]
    go = torch.randn(B, feat, generator=g)
    p = MR.random_params(channels, kernels, pools, seed=7, scale=3.0)
    if name == "zero":
        d[:, -3:] = 0
        q[:, 2] = 0
        for l in range(len(channels)):
            p[f"conv_layers.conv {l}.bias"] = p[f"conv_layers.conv {l}.bias"].abs()
    return q, d, go, p


def geometry(name):
    """per layer (C, Cin, k0, k1, H, W, Ho, Wo, ph, pw)"""
    B, Q, D, E, channels, kernels, pools = CASES[name]
    rows, H, W, cin = [], Q, D, 1
    for c, k, pool in zip(channels, kernels, pools):
        rows.append((c, cin, k[0], k[1], H, W, H + k[1] - k[0], W + k[0] - k[1], pool[0], pool[1]))
        H, W, cin = pool[0], pool[1], c
    return rows


def sum_lengths(name):
    """n of the tolerance rule, from the shape: per layer the B Ho Wo (or B ph pw, if larger) pooled contributions a weight
    or bias gradient adds up; for grad_q / grad_d the chains one output passes through, one after the other (their rounding
    errors add, they do not multiply): the max(Q, D) terms of the cosine stage plus, per layer, the C k0 k1 terms of the
    transposed convolution."""
    B, Q, D = CASES[name][:3]
    geo = geometry(name)
    per_layer = [B * max(Ho * Wo, ph * pw) for (_, _, _, _, _, _, Ho, Wo, ph, pw) in geo]
    emb = max(Q, D) + sum(C * k0 * k1 for (C, _, k0, k1, *_r) in geo)
    return per_layer, emb


def tol(g32, g64, n):
    g64 = g64.double()
    c = max(16.0, math.sqrt(n))
    return 4.0 * float((g32.double() - g64).abs().max()) + c * 2.0 ** -24 * float(g64.abs().max()) if g64.numel() else 0.0


def module(name, dtype):
    from matchmaker_amd.matchpyramid import MatchPyramid
    _, _, _, _, channels, kernels, pools = CASES[name]
    p = inputs(name)[3]
    m = MatchPyramid(channels, kernels, pools)
    m.load_state_dict({k: v for k, v in p.items() if k != "pools"}, strict=True)
    return m.to(dtype)


def _convs(m):
    return [x for x in m.conv_layers if isinstance(x, torch.nn.Conv2d)]


def _grads(m, q, d, feats, go):
    (feats * go).sum().backward()
    cs = _convs(m)
    return {"features": feats.detach(), "gq": q.grad, "gd": d.grad, "gw": [c.weight.grad for c in cs],
            "gb": [c.bias.grad for c in cs]}


@functools.lru_cache(maxsize=None)
def oracle_a(name, dtype):
    """the module's own layers"""
    q, d, go, _ = inputs(name)
    m = module(name, dtype)
    q, d = q.to(dtype).clone().requires_grad_(True), d.to(dtype).clone().requires_grad_(True)
    return _grads(m, q, d, m.torch_features(q, d), go.to(dtype))


def _walk(m, x, pool):
    """the module's layers with `pool(l, relu output, output size)` in place of every AdaptiveMaxPool2d"""
    l = 0
    for layer in m.conv_layers:
        if isinstance(layer, torch.nn.AdaptiveMaxPool2d):
            x = pool(l, x, layer.output_size)
            l += 1
        else:
            x = layer(x)
    return x


def oracle_b(name, dtype, argmax):
    """the given arg-max form; argmax: per layer int64 [B, C, ph pw] flat indices row * Wo + col (not cached: the
    indices are the caller's)"""
    q, d, go, _ = inputs(name)
    m = module(name, dtype)
    q, d = q.to(dtype).clone().requires_grad_(True), d.to(dtype).clone().requires_grad_(True)

    def pool(l, x, size):
        return x.flatten(2).gather(-1, argmax[l]).view(x.shape[0], x.shape[1], size[0], size[1])

    x = _walk(m, m.cosine_module(q, d)[:, None], pool)
    return _grads(m, q, d, x.reshape(x.shape[0], -1), go.to(dtype))


@functools.lru_cache(maxsize=None)
def planes(name, dtype):
    """-> (relu(conv) per layer [B, C, Ho, Wo], torch's own return_indices per layer int64 [B, C, ph pw]), no gradients"""
    q, d, _, _ = inputs(name)
    m = module(name, dtype)
    R, idx = [], []

    def pool(l, x, size):
        y, i = F.adaptive_max_pool2d(x, size, return_indices=True)
        R.append(x)
        idx.append(i.flatten(2))
        return y

    with torch.no_grad():
        _walk(m, m.cosine_module(q.to(dtype), d.to(dtype))[:, None], pool)
    return R, idx


@functools.lru_cache(maxsize=None)
def forward_tol(name):
    """MR.measured_tol of the values the arg-max compares: the largest over the layers' relu(conv) planes"""
    R32, R64 = planes(name, torch.float32)[0], planes(name, torch.float64)[0]
    return max(MR.measured_tol(a, b) for a, b in zip(R32, R64))


def windows(n, o):
    return [((i * n) // o, -((-(i + 1) * n) // o)) for i in range(o)]


@functools.lru_cache(maxsize=None)
def element_gaps(name):
    """per layer, in fp64: (mx, gap, count) each [B, C, ph, pw]: the window maximum, the maximum minus the largest value
    strictly below it (inf where there is none), and how many window elements attain the maximum"""
    out = []
    for R, (_, _, _, _, _, _, Ho, Wo, ph, pw) in zip(planes(name, torch.float64)[0], geometry(name)):
        B, C = R.shape[:2]
        mx, gap, cnt = R.new_zeros(B, C, ph, pw), R.new_zeros(B, C, ph, pw), torch.zeros(B, C, ph, pw, dtype=torch.int64)
        for i, (r0, r1) in enumerate(windows(Ho, ph)):
            for j, (c0, c1) in enumerate(windows(Wo, pw)):
                v = R[:, :, r0:r1, c0:c1].flatten(2)
                m = v.max(-1, keepdim=True).values
                below = torch.where(v < m, v, torch.full_like(v, -math.inf)).max(-1).values
                mx[:, :, i, j], gap[:, :, i, j], cnt[:, :, i, j] = m[..., 0], m[..., 0] - below, (v == m).sum(-1)
        out.append((mx, gap, cnt))
    return out


def strict_gap_per_pair(name):
    """[B]: over all pooled elements with a positive maximum, the smallest gap"""
    B = CASES[name][0]
    best = torch.full((B,), math.inf, dtype=torch.float64)
    for mx, gap, _ in element_gaps(name):
        g = torch.where(mx > 0, gap, torch.full_like(gap, math.inf)).flatten(1).min(-1).values
        best = torch.minimum(best, g)
    return best
