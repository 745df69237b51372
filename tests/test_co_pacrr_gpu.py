"""GPU tests of the fused CO-PACRR kernels (mm_co_pacrr_fwd / mm_co_pacrr_bwd) and the drop-in module: the real class's
goldens, random sweeps and gradients against the fp64 restatement (tests/co_pacrr_reference.py), bit-equality of the last
view with PACRR's kernel, a training step against the module's own eager modules, determinism, the train()-mode RNG draw
and rank parity.

Tolerances as tests/test_pacrr_gpu.py: per_query_results at 2e-5, scores at util.TOL_FP32, gradients at 1e-4 of the largest
component.  Context slots follow the tie rules of DESIGN.md §3.8 (co_pacrr_reference.compare_context_slots)."""
import numpy as np
import pytest
import torch

from matchmaker_amd import ops
from tests import co_pacrr_reference as CP
from tests import util

pytestmark = pytest.mark.gpu

TOL_PQR = 2e-5
TIE_DEPENDENT = {"qpad"}     # see tests/test_co_pacrr_cpu.py


def _params(g, C, N, dev, scale=0.3):
    ws = [(torch.randn(C, 1, n, n, generator=g) * scale).to(dev) for n in range(2, N + 1)]
    bs = [(torch.randn(C, generator=g) * 0.1).to(dev) for _ in range(2, N + 1)]
    return ws, bs


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _value_mask(k, N):
    m = torch.zeros(8 * k * N, dtype=torch.bool)
    for p in range(N):
        m[p * 8 * k:p * 8 * k + 4 * k] = True
    return m


def _load_module(g, dev):
    from matchmaker_amd.co_pacrr import CO_PACRR
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    m = CO_PACRR(Q, int(g["U"]), N, C, k)
    m.load_state_dict({k_[len("param."):]: torch.tensor(v) for k_, v in g.items() if k_.startswith("param.")}, strict=True)
    return m.to(dev).eval()


def _fp64(q, d, ws, bs, k, U, ppq=1):
    q64, d64 = q.double().requires_grad_(True), d.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws]
    b64 = [b.double().requires_grad_(True) for b in bs]
    ref = CP.per_query_results(q64, d64, w64, b64, k, U, ppq)
    mats = CP.paths(q64.detach(), d64.detach(), [w.detach() for w in w64], [b.detach() for b in b64], ppq)
    return q64, d64, w64, b64, ref, mats


@pytest.mark.parametrize("name", ["ref", "short", "mid", "long", "oddu", "padded", "qpad", "b1", "n1", "k1"])
def test_dropin_matches_the_real_class_goldens(name):
    dev = util.require_gpu()
    g = util.load(f"co_pacrr_{name}.npz")
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    U = int(g["U"])
    m = _load_module(g, dev)
    q = torch.tensor(g["q"], device=dev)
    d = torch.tensor(g["d"], device=dev)
    ones_q, ones_d = torch.ones(B, Q, device=dev), torch.ones(B, D, device=dev)
    with torch.no_grad():
        pqr = m.per_query_results(q, d)
        s, sec = m(q, d, ones_q, ones_d, ones_q[..., None], ones_d[..., None], output_secondary_output=True)
    assert s.shape == (B,) and sec == {}
    ref = torch.tensor(g["per_query_results"])
    vm = _value_mask(k, N)
    np.testing.assert_allclose(pqr[..., vm].cpu().numpy(), ref[..., vm].numpy(), rtol=0, atol=TOL_PQR)
    ws, bs = m._conv_params()
    q64, d64, w64, b64, r64, mats = _fp64(q, d, [w.detach() for w in ws], [b.detach() for b in bs], k, U)
    n_ex = CP.compare_context_slots(pqr, r64, mats, k, U, atol=TOL_PQR)            # same tie rule: fp64 decides
    n_ex_real = CP.compare_context_slots(pqr, ref, mats, k, U, atol=TOL_PQR)       # the real class's own ties
    print(f"co_pacrr_{name}: context slots excluded {n_ex} (fp64 restatement) / {n_ex_real} (real class)")
    qg, dg = q.clone().requires_grad_(True), d.clone().requires_grad_(True)
    m.zero_grad()
    m(qg, dg, ones_q, ones_d, ones_q[..., None], ones_d[..., None]).sum().backward()
    assert torch.isfinite(qg.grad).all() and torch.isfinite(dg.grad).all()
    if name in TIE_DEPENDENT:
        # the real class's tie choices move its score and gradients: the drop-in is held to the restatement instead
        dense = [m.dense.weight, m.dense.bias, m.dense2.weight, m.dense2.bias, m.dense3.weight]
        s64 = CP.score(r64, *[t.detach().double() for t in dense])
        np.testing.assert_allclose(s.cpu().numpy(), s64.detach().cpu().numpy(), rtol=0, atol=util.TOL_FP32)
        s64.sum().backward()
        assert _rel(qg.grad, q64.grad) < 1e-4 and _rel(dg.grad, d64.grad) < 1e-4
        for i in range(N - 1):
            assert _rel(m.convolutions[i][1].weight.grad, w64[i].grad) < 1e-4
            assert _rel(m.convolutions[i][1].bias.grad, b64[i].grad) < 1e-4
        return
    np.testing.assert_allclose(s.cpu().numpy(), g["score"], rtol=0, atol=util.TOL_FP32)
    for i in range(N - 1):
        for kind in ("weight", "bias"):
            got = getattr(m.convolutions[i][1], kind).grad
            assert _rel(got, torch.tensor(g[f"grad.convolutions.{i}.1.{kind}"])) < 1e-4, (name, i, kind)
    assert _rel(qg.grad, torch.tensor(g["grad_q"])) < 1e-4
    assert _rel(dg.grad, torch.tensor(g["grad_d"])) < 1e-4


# (n_queries, pairs_per_query, B, Q, U, D, E, C, N, k): D below, between and above the views; every limit edge
SWEEP = [
    (3, 1, 3, 30, 200, 200, 300, 32, 3, 5),
    (2, 1, 2, 30, 200, 37, 64, 16, 3, 5),          # D < v_0
    (2, 1, 2, 30, 200, 120, 64, 16, 3, 5),         # v_1 < D < v_2
    (2, 1, 2, 30, 200, 263, 64, 16, 3, 5),         # D > U
    (2, 1, 2, 17, 30, 45, 64, 16, 4, 7),           # odd U: 7 / 15 / 22 / 30
    (2, 1, 2, 64, 2048, 2048, 64, 8, 2, 8),        # Q, D, k at their limits
    (2, 1, 2, 8, 100, 100, 1024, 64, 5, 8),        # E, C, N at their limits
    (2, 1, 2, 1, 4, 9, 64, 8, 2, 1),               # Q = 1, k = 1, views 1 / 2 / 3 / 4
    (1, 1000, 1000, 30, 200, 200, 300, 32, 3, 5),  # shared query tile
    (3, 60, 130, 20, 64, 70, 36, 16, 3, 4),        # pairs_per_query, last group partial, D > U
]


@pytest.mark.parametrize("nq, ppq, B, Q, U, D, E, C, N, k", SWEEP)
def test_random_sweep_forward_and_backward_against_fp64(nq, ppq, B, Q, U, D, E, C, N, k):
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(Q * 7 + D + E + C + N + k + U)
    q = torch.randn(nq, Q, E, generator=g).to(dev)
    d = torch.randn(B, D, E, generator=g).to(dev)
    ws, bs = _params(g, C, N, dev)
    views = ops.co_pacrr_views(U)
    out, idx = ops.co_pacrr_kmax(q, d, ws, bs, k, views, ppq, save=True)
    assert tuple(out.shape) == (B, Q, 8 * k * N) and tuple(idx.shape) == (B, Q, N, 4 * k)
    q64, d64, w64, b64, ref, mats = _fp64(q, d, ws, bs, k, U, ppq)
    vm = _value_mask(k, N)
    assert float((out[..., vm].double().cpu() - ref.detach()[..., vm].cpu()).abs().max()) < TOL_PQR
    n_ex, tied = CP.compare_context_slots(out, ref, mats, k, U, atol=TOL_PQR, return_pairs=True)
    assert n_ex <= 0.001 * out.numel() / 2
    gout = torch.randn(out.shape, generator=g).to(dev)
    gout[tied.to(dev)] = 0.0     # a pair with a near-tie across the k-th place may route its gradient to another column
    (ref * gout.double()).sum().backward()
    gq, gd, gw, gb = ops.co_pacrr_kmax_bwd(q, d, ws, idx, gout, k, views, ppq)
    for t in [gq, gd] + gw + gb:
        assert torch.isfinite(t).all()
    assert _rel(gq, q64.grad) < 1e-4 and _rel(gd, d64.grad) < 1e-4
    for a, b in zip(gw + gb, w64 + b64):
        assert _rel(a, b.grad) < 1e-4


@pytest.mark.parametrize("D", [120, 200])
def test_last_view_equals_pacrr_bit_for_bit(D):
    """With D <= U the last view is PACRR's whole row: the same cosine / conv / top-k code gives the same bits."""
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(D)
    q = torch.randn(2, 30, 300, generator=g).to(dev)
    d = torch.randn(2000, D, 300, generator=g).to(dev)
    ws, bs = _params(g, 32, 3, dev)
    k, N = 5, 3
    co = ops.co_pacrr_kmax(q, d, ws, bs, k, ops.co_pacrr_views(200), 1000).view(2000, 30, N, 8 * k)
    pa = ops.pacrr_kmax(q, d, ws, bs, k, 1000).view(2000, 30, N, k)
    assert torch.equal(co[..., 3 * k:4 * k], pa)


def _eager_per_query_results(m, q, d):
    """co_pacrr.py:90-158 through the module's own Sequentials, its doc_context_pool and torch.topk (GPU eager)."""
    cos = CP.cosine(q, d)[:, None]
    ctx = CP.cosine(q.mean(dim=1, keepdim=True), m.doc_context_pool(d.transpose(1, 2)).transpose(1, 2))[:, 0]
    out = []
    for path in [cos] + [conv(cos) for conv in m.convolutions]:
        vals, cols = [], []
        for v in m.kmax_pooling_views:
            val, c = torch.topk(path.squeeze(1)[:, :, 0:v], k=m.kmax_pooling_size, sorted=True)
            vals.append(val)
            cols.append(c)
        c = torch.cat(cols, dim=-1)
        out.append(torch.cat(vals + [torch.gather(ctx[:, None].expand(-1, c.shape[1], -1), -1, c)], dim=-1))
    return torch.cat(out, dim=-1)


def test_training_step_matches_the_eager_modules():
    dev = util.require_gpu()
    from matchmaker_amd.co_pacrr import CO_PACRR
    torch.manual_seed(5)
    m = CO_PACRR(30, 200, 3, 32, 5).to(dev).eval()
    B = 64
    q = torch.randn(B, 30, 300, device=dev)
    d = torch.randn(B, 200, 300, device=dev)
    ones_q, ones_d = torch.ones(B, 30, device=dev), torch.ones(B, 200, device=dev)
    loss = m(q, d, ones_q, ones_d, ones_q[..., None], ones_d[..., None]).square().mean()
    loss.backward()
    native = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    pqr = _eager_per_query_results(m, q, d)
    x = torch.relu(m.dense(pqr.view(B, -1)))
    eager = m.dense3(torch.relu(m.dense2(x))).squeeze(1).square().mean()
    eager.backward()
    assert abs(loss.item() - eager.item()) <= 1e-5 * max(1.0, abs(eager.item()))
    for n, p in m.named_parameters():
        assert _rel(native[n], p.grad) < 1e-3, (n, _rel(native[n], p.grad))


def test_determinism_and_inference_equals_training_output():
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(3)
    q = torch.randn(4, 30, 300, generator=g).to(dev)
    d = torch.randn(4000, 200, 300, generator=g).to(dev)
    ws, bs = _params(g, 32, 3, dev)
    v = ops.co_pacrr_views(200)
    a = ops.co_pacrr_kmax(q, d, ws, bs, 5, v, 1000)
    b = ops.co_pacrr_kmax(q, d, ws, bs, 5, v, 1000)
    c, idx = ops.co_pacrr_kmax(q, d, ws, bs, 5, v, 1000, save=True)
    assert torch.equal(a, b) and torch.equal(a, c)
    t, _ = torch.ops.mm_native.co_pacrr_kmax(q, d, ws, bs, 5, v, 1000)
    assert torch.equal(a, t)
    go = torch.randn(c.shape, generator=g).to(dev)
    qq = q[:1].expand(8, -1, -1).contiguous()
    g1 = ops.co_pacrr_kmax_bwd(qq, d[:8], ws, idx[:8], go[:8], 5, v)
    g2 = ops.co_pacrr_kmax_bwd(qq, d[:8], ws, idx[:8], go[:8], 5, v)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    assert all(torch.equal(x, y) for x, y in zip(g1[2] + g1[3], g2[2] + g2[3]))


def test_train_mode_scores_equal_eval_and_the_cpu_rng_advances_as_the_reference():
    dev = util.require_gpu()
    from matchmaker_amd.co_pacrr import CO_PACRR
    torch.manual_seed(1)
    m = CO_PACRR(30, 200, 3, 32, 5).to(dev)
    B = 8
    q, d = torch.randn(B, 30, 300, device=dev), torch.randn(B, 200, 300, device=dev)
    args = (q, d, torch.ones(B, 30, device=dev), torch.ones(B, 200, device=dev), torch.ones(B, 30, 1, device=dev),
            torch.ones(B, 200, 1, device=dev))
    with torch.no_grad():
        s_eval = m.eval()(*args)
        torch.manual_seed(77)
        s_train = m.train()(*args)
        after = torch.rand(4)
    torch.manual_seed(77)
    torch.randperm(30)                  # the reference's one draw (co_pacrr.py:166)
    assert torch.equal(after, torch.rand(4))
    assert torch.equal(s_eval, s_train)
    torch.manual_seed(77)                # eval() draws nothing
    with torch.no_grad():
        m.eval()(*args)
    after_eval = torch.rand(4)
    torch.manual_seed(77)
    assert torch.equal(after_eval, torch.rand(4))


def test_rank_parity_16_queries_x_1000_candidates():
    """Ranks every query's candidates as the reference's fp32 / fp64 arithmetic would.  A near-tie in a top-k list
    swaps a selected column and so a CONTEXT value: the score of such a pair jumps by far more than the
    arithmetic noise between implementations, so those pairs (about a fifth of them here: the conv paths of an untrained
    model cluster on the largest bias) are left out of the ranking and counted."""
    dev = util.require_gpu()
    from matchmaker_amd.co_pacrr import CO_PACRR
    torch.manual_seed(9)
    m = CO_PACRR(30, 200, 3, 32, 5).to(dev).eval()
    nq, ppq, Q, D, E = 16, 1000, 30, 200, 300
    q = torch.randn(nq, Q, E, device=dev)
    dense = [m.dense.weight, m.dense.bias, m.dense2.weight, m.dense2.bias, m.dense3.weight]
    ws, bs = m._conv_params()
    w64, b64 = [w.double() for w in ws], [b.double() for b in bs]
    v = m.kmax_pooling_views
    n_tied = 0
    with torch.no_grad():
        for i in range(nq):
            d = torch.randn(ppq, D, E, device=dev)
            out = ops.co_pacrr_kmax(q[i:i + 1], d, ws, bs, 5, v, ppq)
            p64 = CP.per_query_results(q[i:i + 1].double(), d.double(), w64, b64, 5, 200, ppq)
            mats = CP.paths(q[i:i + 1].double(), d.double(), w64, b64, ppq)
            _, tied = CP.compare_context_slots(out, p64, mats, 5, 200, atol=TOL_PQR, return_pairs=True)
            keep = ~tied
            n_tied += int(tied.sum())
            got = CP.score(out, *dense)[keep].cpu()
            r32 = CP.score(CP.per_query_results(q[i:i + 1], d, ws, bs, 5, 200, ppq), *dense)[keep].cpu()
            r64 = CP.score(p64, *[t.double() for t in dense])[keep].cpu()
            r = util.rank_parity(got.numpy(), r32.numpy(), r64.numpy(), label=f"co_pacrr q{i}")
            # rank_parity asserts every pair further apart than the measured noise.  An untrained model's scores lie
            # close together and a context slot turns a value-level near-tie into a score step, so the undecided
            # positions are more than PACRR's 1 %: on those the device must still match the fp32 sort for 95 %
            assert r["identical_positions_vs_fp32_sort"] >= 0.95 * r["n"], (i, r)
    print(f"co_pacrr rank parity: {n_tied} of {nq * ppq} pairs hold a near-tied group in a top-k list (left out)")
    assert n_tied <= 0.9 * nq * ppq
