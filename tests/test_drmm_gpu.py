"""GPU tests of the fused DRMM kernel (mm_drmm_fwd) and the drop-in module: the real class's goldens, random sweeps to
every stated limit, the fused head, determinism, layout and shortcut bit-equalities, training, rank order and
graph capture (no host synchronisation).

Histograms follow the decided-element rule of DESIGN.md §3.9 (tests/drmm_reference.py): tol = 4 x max |c32 - c64| of the
CPU restatement, at most 0.5 % of the elements of non-padded query rows undecided (asserted first), equality on strict
cases.  Fused scores against the fp64 head on the kernel's own histogram: 1e-5 absolute."""
import numpy as np
import pytest
import torch

from matchmaker_amd import ops, NativeError
from tests import drmm_reference as DR
from tests import util
from tests.test_drmm_cpu import CASES, CAP, VecEmbedder, masked_inputs

pytestmark = pytest.mark.gpu

STRICT = [c for c in CASES if c != "planted"]


def _module(g, dev):
    from matchmaker_amd.drmm import DRMM
    B, Q, D, E, bins = (int(x) for x in g["shape"])
    m = DRMM(VecEmbedder(E), bins)
    m.load_state_dict({k[len("param."):]: torch.tensor(v) for k, v in g.items() if k.startswith("param.")}, strict=True)
    return m.to(dev).eval()


def _tokens(g, dev):
    return ({"tokens": torch.tensor(g["q_tokens"]).to(dev), "vecs": torch.tensor(g["q"]).to(dev)},
            {"tokens": torch.tensor(g["d_tokens"]).to(dev), "vecs": torch.tensor(g["d"]).to(dev)})


def _head_params(m):
    l0, l1 = m.matching_classifier._linear_layers
    return l0.weight.detach(), l0.bias.detach(), l1.weight.detach(), l1.bias.detach()


def _head64(hist, gates, W1, b1, w2, b2):
    x = torch.log1p(hist.double().cpu())
    c = torch.tanh(torch.tanh(x @ W1.double().cpu().T + b1.double().cpu()) @ w2.double().cpu().reshape(1, -1).T + b2.double().cpu())
    return (c.squeeze(-1) * gates.double().cpu()).sum(-1)


@pytest.mark.parametrize("name", CASES)
def test_goldens_histogram_and_score(name):
    dev = util.require_gpu()
    g = util.load(f"drmm_{name}.npz")
    B, Q, D, E, bins = (int(x) for x in g["shape"])
    q, d, qm, dm = masked_inputs(g, torch.float32)
    tol = DR.measured_tol(q, d)
    bd = DR.bounds(q, d, bins, tol, q_rows=qm)
    msg = f"drmm_{name}: tol = {tol:.3e}, undecided = {bd['undecided']}, share = {bd['share']:.3e}"
    print(msg)
    assert bd["share"] <= CAP, msg
    hist = ops.drmm_hist(q.to(dev), d.to(dev), bins)
    DR.check_hist(hist, bd, tol, f"drmm_{name}")
    m = _module(g, dev)
    query, document = _tokens(g, dev)
    with torch.no_grad():
        s = m(query, document)
    assert tuple(s.shape) == (B, 1)
    if int(g["strict"]):
        assert bd["undecided"] == 0, msg
        assert torch.equal(hist.cpu(), torch.tensor(g["hist"])), msg
        np.testing.assert_allclose(s.cpu().numpy(), g["score"], rtol=0, atol=1e-5)
    else:
        # the golden's own histogram lost exact matches to rounding: the score is held to the fp64 head on the kernel's histogram
        p = DR.params64(g)
        s64 = DR.head(hist.double().cpu(), DR.gate(q.double(), qm.double(), p), p)
        np.testing.assert_allclose(s.cpu().numpy(), s64.numpy(), rtol=0, atol=1e-5)


# (n_queries, pairs_per_query, B, Q, D, E, bins, lengths): every limit edge, both kernels (E = 100 n streams, the rest direct)
SWEEP = [
    (3, 1, 3, 30, 200, 300, 10, False),
    (2, 1, 2, 32, 200, 100, 10, True),
    (2, 1, 2, 17, 77, 200, 16, True),
    (2, 1, 2, 64, 130, 300, 10, False),             # Q at its limit: the direct kernel with two row tiles
    (2, 1, 2, 64, 90, 1024, 16, True),              # Q, E, bins at their limits
    (2, 1, 2, 33, 45, 768, 1, False),               # one bin
    (1, 1, 1, 5, 65535, 4, 10, True),               # D at its limit, the narrowest E
    (1, 1, 1, 30, 65535, 100, 3, False),            # D at its limit on the stream
    (1, 1000, 1000, 30, 200, 300, 10, True),        # shared query tile
    (3, 60, 130, 20, 70, 36, 7, True),              # pairs_per_query, last group partial
    (2, 1, 2, 1, 1, 64, 10, False),                 # Q = 1, D = 1
]


@pytest.mark.parametrize("nq, ppq, B, Q, D, E, bins, lens", SWEEP)
def test_random_sweep_against_the_decided_bounds(nq, ppq, B, Q, D, E, bins, lens):
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(Q * 7 + D + E + bins + B)
    q = torch.randn(nq, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    d[:, ::13] = 0                                   # OOV rows mid-document
    d_len = None
    if lens:
        d_len = torch.randint(0, D + 1, (B,), generator=g).to(torch.int32)
        d = d * (torch.arange(D)[None, :, None] < d_len[:, None, None]).float()
    tol = DR.measured_tol(q, d, ppq)
    bd = DR.bounds(q, d, bins, tol, ppq)
    msg = f"tol = {tol:.3e}, undecided = {bd['undecided']}, share = {bd['share']:.3e}"
    print(msg)
    assert bd["share"] <= CAP, msg
    hist = ops.drmm_hist(q.to(dev), d.to(dev), bins, ppq)
    assert tuple(hist.shape) == (B, Q, bins)
    DR.check_hist(hist, bd, tol, "sweep")
    if lens:                                         # the padded-tail shortcut is bit-equal to the full computation
        assert torch.equal(hist, ops.drmm_hist(q.to(dev), d.to(dev), bins, ppq, d_len=d_len.to(dev)))
    # fused score: the fp64 head on the kernel's own histogram, and hist mode / score mode bit-consistent
    W1, b1 = torch.randn(bins, bins, generator=g).to(dev), torch.randn(bins, generator=g).to(dev)
    w2, b2 = torch.randn(1, bins, generator=g).to(dev), torch.randn(1, generator=g).to(dev)
    gate = torch.softmax(torch.randn(nq, Q, generator=g), dim=-1).to(dev)
    s, h2 = ops.drmm_score(q.to(dev), d.to(dev), gate, W1, b1, w2, b2, ppq, return_hist=True)
    assert torch.equal(h2, hist)
    assert torch.equal(s, ops.drmm_score(q.to(dev), d.to(dev), gate, W1, b1, w2, b2, ppq))
    gates = DR.expand_queries(gate, B, ppq)
    err = float((s.double().cpu() - _head64(hist, gates, W1, b1, w2, b2)).abs().max())
    assert err <= 1e-5, err
    sp = ops.drmm_score(q.to(dev), d.to(dev), gates.contiguous(), W1, b1, w2, b2, ppq)        # per-pair gate rows
    assert torch.equal(s, sp)


def test_layouts_determinism_and_torch_ops_are_bit_equal():
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(3)
    q = torch.randn(4, 30, 300, generator=g).to(dev)
    d = torch.randn(4000, 200, 300, generator=g).to(dev)
    a = ops.drmm_hist(q, d, 10, 1000)
    assert torch.equal(a, ops.drmm_hist(q, d, 10, 1000))                                         # two runs
    assert torch.equal(a, ops.drmm_hist(q.repeat_interleave(1000, dim=0), d, 10, 1))             # replicated query
    assert torch.equal(a, torch.ops.mm_native.drmm_hist(q, d, 10, 1000))
    assert (a.sum(-1) <= 200).all() and (a.sum(-1) >= 199).all()
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(a, torch.ops.mm_native.drmm_hist(q, d, 10, 1000))                     # inputs stay fp32
    qg = q.clone().requires_grad_(True)
    h = torch.ops.mm_native.drmm_hist(qg, d, 10, 1000)
    assert not h.requires_grad                                                                   # non-differentiable
    # a direct-kernel shape too
    q2, d2 = torch.randn(2, 40, 64, generator=g).to(dev), torch.randn(300, 150, 64, generator=g).to(dev)
    b = ops.drmm_hist(q2, d2, 16, 150)
    assert torch.equal(b, ops.drmm_hist(q2, d2, 16, 150))
    assert torch.equal(b, ops.drmm_hist(q2.repeat_interleave(150, dim=0), d2, 16, 1))


def test_clamp_puts_every_planted_exact_match_in_the_last_bin():
    dev = util.require_gpu()
    g = util.load("drmm_planted.npz")
    B, Q, D, E, bins = (int(x) for x in g["shape"])
    q, d, qm, dm = masked_inputs(g, torch.float32)
    c64 = DR.cosine(q.double(), d.double())
    exact = (c64 > 1 - 1e-9)
    assert int(exact.sum()) > 50
    plain = ops.drmm_hist(q.to(dev), d.to(dev), bins).cpu()
    clamped = ops.drmm_hist(q.to(dev), d.to(dev), bins, clamp=True).cpu()
    inlast = (c64 >= 1 - 2.0 / bins + 1e-5).sum(-1).float()       # decided members of the last bin, exact matches included
    assert torch.equal(clamped[..., -1], inlast)
    assert (clamped.sum(-1) == D).all()                            # nothing is dropped
    assert (plain[..., -1] <= clamped[..., -1]).all() and torch.equal(plain[..., :-1], clamped[..., :-1])


def test_out_of_limit_shapes_raise_before_any_launch():
    dev = util.require_gpu()
    for Q, D, E, bins in [(65, 200, 64, 10), (30, 65536, 4, 10), (30, 200, 1028, 10), (30, 200, 64, 17)]:
        with pytest.raises(NativeError):
            ops.drmm_hist(torch.zeros(1, Q, E, device=dev), torch.zeros(1, D, E, device=dev), bins)
    with pytest.raises(NativeError):
        ops.drmm_hist(torch.zeros(1, 30, 64, device=dev).half(), torch.zeros(1, 200, 64, device=dev).half())
    torch.cuda.synchronize()


def _random_batch(B, Q, D, E, dev, seed):
    g = torch.Generator().manual_seed(seed)
    qt = torch.randint(2, 1000, (B, Q), generator=g) * (torch.arange(Q)[None] < torch.randint(3, Q + 1, (B, 1), generator=g))
    dt = torch.randint(2, 1000, (B, D), generator=g) * (torch.arange(D)[None] < torch.randint(20, D + 1, (B, 1), generator=g))
    dt[:, 5::17] = torch.minimum(dt[:, 5::17], torch.ones_like(dt[:, 5::17]))
    query = {"tokens": qt.to(dev), "vecs": torch.randn(B, Q, E, generator=g).to(dev)}
    document = {"tokens": dt.to(dev), "vecs": torch.randn(B, D, E, generator=g).to(dev)}
    return query, document


def test_dropin_eval_and_train_forward_agree_and_a_training_step_moves_both_feedforwards():
    dev = util.require_gpu()
    from matchmaker_amd.drmm import DRMM
    torch.manual_seed(5)
    m = DRMM(VecEmbedder(300), 10).to(dev)
    query, document = _random_batch(64, 30, 200, 300, dev, 6)
    query["vecs"].requires_grad_(True)
    m.eval()
    with torch.no_grad():
        s_eval = m(query, document)
    m.train()
    s_train = m(query, document)
    assert tuple(s_eval.shape) == (64, 1) and tuple(s_train.shape) == (64, 1)
    assert float((s_eval - s_train.detach()).abs().max()) <= 1e-6
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    s_train.square().mean().backward()
    opt.step()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
        assert not torch.equal(p.detach(), before[n]), n
    # the histogram has no gradient: the query vectors receive theirs through the gate alone, documents none
    assert document["vecs"].grad is None
    hist = torch.ops.mm_native.drmm_hist(query["vecs"], document["vecs"], 10, 1)
    assert not hist.requires_grad


def test_dropin_forward_is_capturable_no_host_synchronisation():
    dev = util.require_gpu()
    from matchmaker_amd.drmm import DRMM
    torch.manual_seed(7)
    m = DRMM(VecEmbedder(300), 10).to(dev).eval()
    query, document = _random_batch(32, 30, 200, 300, dev, 8)
    with torch.no_grad():
        ref = m(query, document)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(query, document)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):          # any .cpu() / .item() / synchronise inside raises during capture
            out = m(query, document)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_rank_order_16_queries_x_1000_candidates():
    dev = util.require_gpu()
    # score noise: the largest |native - golden| score difference over the strict goldens
    noise = 0.0
    for name in STRICT:
        g = util.load(f"drmm_{name}.npz")
        m = _module(g, dev)
        with torch.no_grad():
            s = m(*_tokens(g, dev))
        noise = max(noise, float(np.abs(s.cpu().numpy() - g["score"]).max()))
    noise = max(noise, 1e-7)
    from matchmaker_amd.drmm import DRMM
    torch.manual_seed(9)
    m = DRMM(VecEmbedder(300), 10).to(dev).eval()
    p = {k: v.double().cpu() for k, v in m.state_dict().items()}
    nq, ppq, Q, D, E = 16, 1000, 30, 200, 300
    g = torch.Generator().manual_seed(10)
    q = torch.randn(nq, Q, E, generator=g)
    qm = torch.ones(nq, Q)
    decided_total = 0
    for i in range(nq):
        d = torch.randn(ppq, D, E, generator=g)
        with torch.no_grad():
            got = m.score_embeddings(q[i:i + 1].to(dev), d.to(dev), qm[i:i + 1].to(dev), None, pairs_per_query=ppq)[:, 0].double().cpu()
        tol = DR.measured_tol(q[i:i + 1], d, ppq)
        bd = DR.bounds(q[i:i + 1], d, 10, tol, ppq)
        # candidates with an undecided element have no defined fp64 score: they are left out of the order check
        ok = (bd["total_hi"] == bd["total_lo"]).all(-1)
        s64 = DR.score(q[i:i + 1].double(), d.double(), qm[i:i + 1].double(), p, 10, ppq)[:, 0]
        assert float((got[ok] - s64[ok]).abs().max()) <= max(2 * noise, 1e-5)
        a, b = got[ok].numpy(), s64[ok].numpy()
        order_ref = np.argsort(-b, kind="stable")
        order_got = np.argsort(-a, kind="stable")
        gaps = np.abs(np.diff(b[order_ref]))
        big = gaps > noise
        dec = np.concatenate([[True], big]) & np.concatenate([big, [True]])
        assert (order_ref[dec] == order_got[dec]).all(), f"query {i}: a decided rank position differs (noise {noise:.3e})"
        decided_total += int(dec.sum())
    print(f"rank order: score noise {noise:.3e}, {decided_total} decided positions of {nq * ppq}")
    assert decided_total > 0
