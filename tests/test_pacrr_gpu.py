"""GPU tests of the fused PACRR kernels (mm_pacrr_fwd / mm_pacrr_bwd) and the drop-in module: the real class's goldens,
random sweeps and gradients against the fp64 restatement (tests/pacrr_reference.py), a training step against the module's
own eager Sequentials, rank parity at the reference shape, determinism, and the limits.

Tolerances.  The cosine's dot runs on the exact-fp32 MFMA (a k-ordered fma chain: error <= ~1.5e-7 sum|q_e d_e|, i.e. a few
1e-7 on a cosine of unit vectors, measured 4e-8 .. 1.8e-7 against fp64 over the sweep below), the conv is an fp32 fma chain
of n^2 <= 25 taps over those cosines: |err| <= sum|w| * 2e-7 + n^2 ulp(|value|) ~ 1e-6 for |w| <= 1.  per_query_results are
checked at 2e-5 (10x that bound), scores (three fp32 dense layers on top) at util.TOL_FP32 = 1e-3 as the ceiling, 1e-4 in
practice.  Gradients are sums of O(Q k) such terms: relative 1e-4 of the largest component."""
import numpy as np
import pytest
import torch

from matchmaker_amd import NativeError, ops
from tests import pacrr_reference as P
from tests import util

pytestmark = pytest.mark.gpu

TOL_PQR = 2e-5


def _params(g, C, N, dev, scale=0.3):
    ws = [(torch.randn(C, 1, n, n, generator=g) * scale).to(dev) for n in range(2, N + 1)]
    bs = [(torch.randn(C, generator=g) * 0.1).to(dev) for _ in range(2, N + 1)]
    return ws, bs


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _load_module(g, dev):
    from matchmaker_amd.pacrr import PACRR
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    m = PACRR(Q, D, N, C, k)
    m.load_state_dict({k_[len("param."):]: torch.tensor(v) for k_, v in g.items() if k_.startswith("param.")}, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("name", ["ref", "b1", "q1", "n1", "n4", "k1", "padded"])
def test_dropin_matches_the_real_class_goldens(name):
    dev = util.require_gpu()
    g = util.load(f"pacrr_{name}.npz")
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    m = _load_module(g, dev)
    q = torch.tensor(g["q"], device=dev)
    d = torch.tensor(g["d"], device=dev)
    ones_q, ones_d = torch.ones(B, Q, device=dev), torch.ones(B, D, device=dev)
    with torch.no_grad():
        pqr = m.per_query_results(q, d)
        s = m(q, d, ones_q, ones_d, ones_q[..., None], ones_d[..., None], output_secondary_output=True)
    assert s.shape == (B,)
    np.testing.assert_allclose(pqr.cpu().numpy(), g["per_query_results"], rtol=0, atol=TOL_PQR)
    np.testing.assert_allclose(s.cpu().numpy(), g["score"], rtol=0, atol=util.TOL_FP32)
    # training: gradients of score.sum() through the autograd rule
    qg, dg = q.clone().requires_grad_(True), d.clone().requires_grad_(True)
    m.zero_grad()
    m(qg, dg, ones_q, ones_d, ones_q[..., None], ones_d[..., None]).sum().backward()
    for i in range(N - 1):
        for kind in ("weight", "bias"):
            got = getattr(m.convolutions[i][1], kind).grad
            ref = torch.tensor(g[f"grad.convolutions.{i}.1.{kind}"])
            assert _rel(got, ref) < 1e-4, (name, i, kind, _rel(got, ref))
    gq, gd = qg.grad.cpu(), dg.grad.cpu()
    assert torch.isfinite(gq).all() and torch.isfinite(gd).all()
    assert _rel(gq, torch.tensor(g["grad_q"])) < 1e-4
    lens = g["doc_len"] if "doc_len" in g else np.full(B, D)
    pad = torch.tensor(np.arange(D)[None, :] >= lens[:, None])
    ref_gd = torch.tensor(g["grad_d"])
    assert _rel(gd[~pad], ref_gd[~pad]) < 1e-4
    for b in range(B):               # padded rows tie exactly: compared as their sum (tie policy)
        if pad[b].any():
            assert _rel(gd[b][pad[b]].sum(0), ref_gd[b][pad[b]].sum(0)) < 1e-4


# (n_queries, pairs_per_query, B, Q, D, E, C, N, k): every value of each sweep axis appears at least once
SWEEP = [
    (3, 1, 3, 30, 200, 300, 32, 3, 5),
    (2, 1, 2, 1, 33, 64, 16, 2, 5),
    (2, 1, 2, 20, 511, 768, 64, 5, 16),
    (2, 1, 2, 64, 2048, 64, 32, 3, 16),
    (1, 1000, 1000, 30, 200, 300, 32, 3, 5),
    (2, 1, 2, 30, 16, 64, 16, 1, 16),          # D = k
    (2, 1, 2, 64, 1, 768, 64, 2, 1),           # D = k = 1
    (2, 1000, 1500, 20, 33, 64, 16, 3, 5),
    (2, 1, 2, 30, 200, 300, 64, 5, 1),
]


@pytest.mark.parametrize("nq, ppq, B, Q, D, E, C, N, k", SWEEP)
def test_random_sweep_forward_and_backward_against_fp64(nq, ppq, B, Q, D, E, C, N, k):
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(Q * 7 + D + E + C + N + k)
    q = torch.randn(nq, Q, E, generator=g).to(dev)
    d = torch.randn(B, D, E, generator=g).to(dev)
    ws, bs = _params(g, C, N, dev)
    out, idx = ops.pacrr_kmax(q, d, ws, bs, k, ppq, save=True)
    q64, d64 = q.double().requires_grad_(True), d.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws]
    b64 = [b.double().requires_grad_(True) for b in bs]
    ref, cols, chans = P.per_query_results(q64, d64, w64, b64, k, ppq, return_positions=True)
    assert tuple(out.shape) == (B, Q, k * N)
    assert float((out.double() - ref.detach()).abs().max()) < TOL_PQR
    # positions: identical wherever fp64 separates the neighbours (random data: everywhere)
    assert float(((idx.long() & 0xffff) == cols).double().mean()) > 0.999
    assert float(((idx.long() >> 16) == chans).double().mean()) > 0.999
    gout = torch.randn(out.shape, generator=g).to(dev)
    (ref * gout.double()).sum().backward()
    gq, gd, gw, gb = ops.pacrr_kmax_bwd(q, d, ws, idx, gout, k, ppq)
    for t in [gq, gd] + gw + gb:
        assert torch.isfinite(t).all()
    assert _rel(gq, q64.grad) < 1e-4 and _rel(gd, d64.grad) < 1e-4
    for a, b in zip(gw, w64):
        assert _rel(a, b.grad) < 1e-4
    for a, b in zip(gb, b64):
        assert _rel(a, b.grad) < 1e-4


def test_zero_padded_documents_backward_and_the_tie_policy():
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(11)
    B, Q, D, E, C, N, k = 4, 30, 200, 300, 32, 3, 16
    lens = torch.tensor([200, 90, 40, 17])          # 17 < k + 2: zero columns enter the top-k of path 0 (exact ties)
    q = torch.randn(B, Q, E, generator=g).to(dev)
    d = (torch.randn(B, D, E, generator=g) * (torch.arange(D)[None, :, None] < lens[:, None, None])).to(dev)
    ws, bs = _params(g, C, N, dev)
    out, idx = ops.pacrr_kmax(q, d, ws, bs, k, save=True)
    q64, d64 = q.double().requires_grad_(True), d.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws]
    b64 = [b.double().requires_grad_(True) for b in bs]
    ref, cols, _ = P.per_query_results(q64, d64, w64, b64, k, return_positions=True)
    assert float((out.double() - ref.detach()).abs().max()) < TOL_PQR
    gout = torch.randn(out.shape, generator=g).to(dev)
    (ref * gout.double()).sum().backward()
    gq, gd, gw, gb = ops.pacrr_kmax_bwd(q, d, ws, idx, gout, k)
    assert all(torch.isfinite(t).all() for t in [gq, gd] + gw + gb)
    pad = (torch.arange(D)[None, :] >= lens[:, None]).to(dev)
    assert _rel(gq, q64.grad) < 1e-4
    assert _rel(gd[~pad], d64.grad[~pad]) < 1e-4
    for b in range(B):
        if pad[b].any():
            assert _rel(gd[b][pad[b]].sum(0), d64.grad[b][pad[b]].sum(0)) < 1e-4
    for a, b in zip(gw + gb, w64 + b64):
        assert _rel(a, b.grad) < 1e-4


def test_training_step_matches_the_eager_modules():
    """loss.backward() through the drop-in gives the parameter gradients of the module's own Sequentials + torch.topk."""
    dev = util.require_gpu()
    from matchmaker_amd.pacrr import PACRR
    torch.manual_seed(5)
    m = PACRR(30, 200, 3, 32, 5).to(dev)
    B = 64
    q = torch.randn(B, 30, 300, device=dev)
    d = torch.randn(B, 200, 300, device=dev)
    ones_q, ones_d = torch.ones(B, 30, device=dev), torch.ones(B, 200, device=dev)
    loss = m(q, d, ones_q, ones_d, ones_q[..., None], ones_d[..., None]).square().mean()
    loss.backward()
    native = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    cos = P.cosine(q, d)[:, None]
    res = [torch.topk(cos.squeeze(1), k=5, sorted=True)[0]]
    for conv in m.convolutions:
        res.append(torch.topk(conv(cos).squeeze(1), k=5, sorted=True)[0])
    pqr = torch.cat(res, dim=-1)
    x = torch.relu(m.dense(pqr.view(B, -1)))
    eager = m.dense3(torch.relu(m.dense2(x))).squeeze(1).square().mean()
    eager.backward()
    assert abs(loss.item() - eager.item()) <= 1e-5 * max(1.0, abs(eager.item()))
    for n, p in m.named_parameters():
        assert _rel(native[n], p.grad) < 1e-3, (n, _rel(native[n], p.grad))


def test_rank_parity_16_queries_x_1000_candidates():
    dev = util.require_gpu()
    from matchmaker_amd.pacrr import PACRR
    torch.manual_seed(9)
    m = PACRR(30, 200, 3, 32, 5).to(dev).eval()
    nq, ppq, Q, D, E = 16, 1000, 30, 200, 300
    q = torch.randn(nq, Q, E, device=dev)
    got, r32, r64 = [], [], []
    dense = [m.dense.weight, m.dense.bias, m.dense2.weight, m.dense2.bias, m.dense3.weight]
    ws, bs = m._conv_params()
    with torch.no_grad():
        for i in range(nq):
            d = torch.randn(ppq, D, E, device=dev)
            got.append(P.score(ops.pacrr_kmax(q[i:i + 1], d, ws, bs, 5, ppq), *dense).cpu())
            r32.append(P.score(P.per_query_results(q[i:i + 1], d, ws, bs, 5, ppq), *dense).cpu())
            r64.append(P.score(P.per_query_results(q[i:i + 1].double(), d.double(), [w.double() for w in ws],
                                                   [b.double() for b in bs], 5, ppq), *[t.double() for t in dense]).cpu())
    rows = []
    for i in range(nq):
        rows.append(util.rank_parity(got[i].numpy(), r32[i].numpy(), r64[i].numpy(), label=f"pacrr q{i}"))
    # rank_parity asserts the order of every pair further apart than the measured noise; an untrained model's scores are
    # close together, so a few per cent of the positions are undecided ties — on those the device must still match the
    # reference's own fp32 ranking (the stable sort its metrics code applies)
    for i, r in enumerate(rows):
        assert r["identical_positions_vs_fp32_sort"] >= 0.99 * r["n"], (i, r)


def test_determinism_and_inference_equals_training_output():
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(3)
    q = torch.randn(4, 30, 300, generator=g).to(dev)
    d = torch.randn(4000, 200, 300, generator=g).to(dev)
    ws, bs = _params(g, 32, 3, dev)
    a = ops.pacrr_kmax(q, d, ws, bs, 5, 1000)
    b = ops.pacrr_kmax(q, d, ws, bs, 5, 1000)
    c, idx = ops.pacrr_kmax(q, d, ws, bs, 5, 1000, save=True)
    assert torch.equal(a, b) and torch.equal(a, c)
    t, _ = torch.ops.mm_native.pacrr_kmax(q, d, ws, bs, 5, 1000)
    assert torch.equal(a, t)
    go = torch.randn(c.shape, generator=g).to(dev)
    g1 = ops.pacrr_kmax_bwd(q[:1].expand(8, -1, -1).contiguous(), d[:8], ws, idx[:8], go[:8], 5)
    g2 = ops.pacrr_kmax_bwd(q[:1].expand(8, -1, -1).contiguous(), d[:8], ws, idx[:8], go[:8], 5)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    assert all(torch.equal(x, y) for x, y in zip(g1[2] + g1[3], g2[2] + g2[3]))


@pytest.mark.parametrize("Q, D, E, C, N, k", [(65, 200, 64, 32, 3, 5), (30, 2049, 64, 32, 3, 5), (30, 200, 1028, 32, 3, 5),
                                              (30, 200, 64, 65, 3, 5), (30, 200, 64, 32, 6, 5), (30, 200, 64, 32, 3, 33),
                                              (30, 4, 64, 32, 3, 5)])
def test_out_of_limit_shapes_raise_before_any_launch(Q, D, E, C, N, k):
    dev = util.require_gpu()
    q = torch.zeros(2, Q, E, device=dev)
    d = torch.zeros(2, D, E, device=dev)
    ws = [torch.zeros(C, 1, n, n, device=dev) for n in range(2, N + 1)]
    bs = [torch.zeros(C, device=dev) for _ in range(2, N + 1)]
    with pytest.raises(NativeError):
        ops.pacrr_kmax(q, d, ws, bs, k)
    torch.cuda.synchronize()
