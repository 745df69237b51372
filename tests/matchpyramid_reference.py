"""Restatement of MatchPyramid's forward (matchmaker/models/matchpyramid.py:74-107) from its behaviour, in torch ops and
parametrised by dtype: the fp64 run is the yardstick of the GPU tests, the fp32 run measures what an fp32 evaluation loses.

    cosine   x / (|x| + 1e-13) on both sides, then the dot products; no mask enters
    layer    zero columns on the right (k[0] - 1) and zero rows below (k[1] - 1), a k[0]-row x k[1]-column cross-correlation
             plus bias at every output position, max(0, .), adaptive max pooling whose output i along an axis of length n
             covers [floor(i n / o), ceil((i + 1) n / o))
    head     relu(dense) -> relu(dense2) -> dense3 (no bias) -> [B]

params: {"conv_layers.conv <i>.weight" | ".bias", "dense.weight", ...} (state_dict keys) plus "pools": [(ph, pw), ...]."""
import math

import torch

DEFAULT = ([16, 16, 16, 16, 16], [[3, 3]] * 5, [[36, 90], [18, 60], [9, 30], [6, 20], [3, 10]])


def n_layers(params):
    return len(params["pools"])


def cosine(q, d):
    qn = q / (q.pow(2).sum(-1, keepdim=True).sqrt() + 1e-13)
    dn = d / (d.pow(2).sum(-1, keepdim=True).sqrt() + 1e-13)
    return qn @ dn.transpose(-1, -2)


def adaptive_max(x, oh, ow):
    B, C, H, W = x.shape
    rows = []
    for i in range(oh):
        r0, r1 = (i * H) // oh, -((-(i + 1) * H) // oh)
        band = x[:, :, r0:r1].amax(dim=2)
        rows.append(torch.stack([band[:, :, (j * W) // ow:-((-(j + 1) * W) // ow)].amax(dim=2) for j in range(ow)], dim=-1))
    return torch.stack(rows, dim=2)


def conv_layer(x, w, b):
    """zero pad right by k0 - 1 and below by k1 - 1, then a k0 x k1 cross-correlation (unfold + matmul) plus bias"""
    C, Cin, k0, k1 = w.shape
    B, _, H, W = x.shape
    xp = x.new_zeros(B, Cin, H + k1 - 1, W + k0 - 1)
    xp[:, :, :H, :W] = x
    Ho, Wo = H + k1 - k0, W + k0 - k1
    out = b.view(1, C, 1, 1).expand(B, C, Ho, Wo).clone()
    for a in range(k0):
        for c in range(k1):
            out = out + torch.einsum("oc,bchw->bohw", w[:, :, a, c], xp[:, :, a:a + Ho, c:c + Wo])
    return out


def pyramid(q, d, params, dtype, pairs_per_query=1, upto=None):
    """pooled output of layer `upto` (default: the last) [B, C, ph, pw]; q [nq, Q, E], d [B, D, E]"""
    q, d = q.to(dtype), d.to(dtype)
    if pairs_per_query > 1:
        q = q.repeat_interleave(pairs_per_query, dim=0)[:d.shape[0]]
    x = cosine(q, d)[:, None]
    L = n_layers(params)
    for l in range(L if upto is None else upto + 1):
        w, b = params[f"conv_layers.conv {l}.weight"].to(dtype), params[f"conv_layers.conv {l}.bias"].to(dtype)
        x = adaptive_max(conv_layer(x, w, b).clamp_min(0), *params["pools"][l])
    return x


def features(q, d, params, dtype, pairs_per_query=1):
    x = pyramid(q, d, params, dtype, pairs_per_query)
    return x.reshape(x.shape[0], -1)


def head(feat, params, dtype):
    x = torch.relu(feat.to(dtype) @ params["dense.weight"].to(dtype).T + params["dense.bias"].to(dtype))
    x = torch.relu(x @ params["dense2.weight"].to(dtype).T + params["dense2.bias"].to(dtype))
    return (x @ params["dense3.weight"].to(dtype).T).squeeze(1)


def score(q, d, params, dtype, pairs_per_query=1):
    return head(features(q, d, params, dtype, pairs_per_query), params, dtype)


def measured_tol(x32, x64):
    """4 x the fp32 restatement's own error against fp64 (DESIGN.md §3.9's factor) + 16 ulps of the largest activation (a
    k-ordered fp32 chain of up to 32 x 25 terms against the CPU's blocked sums: sqrt(n) eps ~ 16 eps)."""
    x64 = x64.double()
    return 4.0 * float((x32.double() - x64).abs().max()) + 16.0 * 2.0 ** -24 * float(x64.abs().max())


def params_from_golden(g):
    p = {k[len("param."):]: torch.tensor(v) for k, v in g.items() if k.startswith("param.")}
    p["pools"] = [tuple(int(x) for x in r) for r in g["pools"]]
    return p


def params_from_module(m):
    p = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    p["pools"] = [tuple(x.output_size) for x in m.conv_layers if isinstance(x, torch.nn.AdaptiveMaxPool2d)]
    return p


def conv_lists(params):
    L = n_layers(params)
    return ([params[f"conv_layers.conv {l}.weight"] for l in range(L)], [params[f"conv_layers.conv {l}.bias"] for l in range(L)])


def random_params(channels, kernels, pools, seed, scale=1.0):
    """conv parameters with Conv2d's default init range (uniform +- 1 / sqrt(fan-in)) times `scale`, and a dense head"""
    g = torch.Generator().manual_seed(seed)
    p, cin = {"pools": [tuple(x) for x in pools]}, 1
    for l, (c, k) in enumerate(zip(channels, kernels)):
        bound = scale / math.sqrt(cin * k[0] * k[1])
        p[f"conv_layers.conv {l}.weight"] = (torch.rand(c, cin, k[0], k[1], generator=g) * 2 - 1) * bound
        p[f"conv_layers.conv {l}.bias"] = (torch.rand(c, generator=g) * 2 - 1) * bound
        cin = c
    feat = cin * pools[-1][0] * pools[-1][1]
    for name, (o, i, bias) in {"dense": (100, feat, True), "dense2": (10, 100, True), "dense3": (1, 10, False)}.items():
        p[name + ".weight"] = (torch.rand(o, i, generator=g) * 2 - 1) / math.sqrt(i)
        if bias:
            p[name + ".bias"] = (torch.rand(o, generator=g) * 2 - 1) / math.sqrt(i)
    return p


# the rank-order list shared by the CPU and GPU tests: one query x 200 candidates
RANK_SHAPE = (1, 200, 8, 20, 16)
RANK_PYRAMID = ([4, 4], [[3, 3], [3, 3]], [[4, 8], [2, 3]])
RANK_SEED = 11


def rank_inputs(seed=RANK_SEED):
    nq, B, Q, D, E = RANK_SHAPE
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nq, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    return q, d, random_params(*RANK_PYRAMID, seed=seed + 1, scale=3.0)


def undecided_share(s64, tol):
    gaps = (s64.double().sort(descending=True).values.diff()).abs()
    return float((gaps <= 2 * tol).double().mean())
