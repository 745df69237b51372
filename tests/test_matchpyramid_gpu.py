"""GPU tests of the fused MatchPyramid kernel (mm_matchpyramid_fwd) and the drop-in module: the real class's goldens, a
random sweep to the stated limits, the generic twin (MM_MP_GENERIC=1, in one child process), determinism and layout
bit-equalities, refusals, the module's dispatch, rank order and graph capture.

Tolerance (tests/matchpyramid_reference.py): the device result against the fp64 restatement within
measured_tol = 4 x max |x32 - x64| + 16 x 2^-24 x max |x64|, x32 the CPU's fp32 restatement.  Every test prints its tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from matchmaker_amd import _lib, ops, NativeError
from tests import matchpyramid_reference as MR
from tests import util
from tests.test_matchpyramid_cpu import CASES, module_from_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _features(q, d, p, dev, ppq=1):
    w, b = MR.conv_lists(p)
    return ops.matchpyramid_features(q.to(dev), d.to(dev), [t.to(dev) for t in w], [t.to(dev) for t in b], p["pools"], ppq)


def _check(got, q, d, p, label, ppq=1):
    f64 = MR.features(q, d, p, torch.float64, ppq)
    tol = MR.measured_tol(MR.features(q, d, p, torch.float32, ppq), f64)
    err = float((got.double().cpu() - f64).abs().max())
    print(f"{label}: tol = {tol:.3e}, err = {err:.3e}, max |features| = {float(f64.abs().max()):.3e}")
    assert tuple(got.shape) == tuple(f64.shape)
    assert err <= tol, (label, err, tol)


@pytest.mark.parametrize("name", CASES)
def test_goldens_features_and_module_score(name):
    dev = util.require_gpu()
    g = util.load(f"matchpyramid_{name}.npz")
    p = MR.params_from_golden(g)
    q, d = torch.tensor(g["q"]), torch.tensor(g["d"])
    got = _features(q, d, p, dev)
    _check(got, q, d, p, f"matchpyramid_{name}")
    m = module_from_golden(g).to(dev).eval()
    with torch.no_grad():
        s = m(q.to(dev), d.to(dev), None, None)
    s64 = MR.score(q, d, p, torch.float64)
    tol = MR.measured_tol(MR.score(q, d, p, torch.float32), s64)
    err = float((s.double().cpu() - s64).abs().max())
    print(f"matchpyramid_{name} score: tol = {tol:.3e}, err = {err:.3e}")
    assert tuple(s.shape) == (q.shape[0],) and err <= tol


def test_generic_twin_is_bit_equal_on_every_golden(tmp_path):
    """MM_MP_GENERIC is read once per process: the generic kernel runs in ONE fresh child"""
    dev = util.require_gpu()
    out = tmp_path / "generic.npz"
    code = ("import sys, numpy as np, torch\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from tests import util, matchpyramid_reference as MR\n"
            "from tests.test_matchpyramid_gpu import _features\n"
            f"res = {{n: _features(torch.tensor(g['q']), torch.tensor(g['d']), MR.params_from_golden(g), torch.device('cuda:0')).cpu().numpy()"
            f" for n in {CASES!r} for g in [util.load(f'matchpyramid_{{n}}.npz')]}}\n"
            f"np.savez({str(out)!r}, **res)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MM_MP_GENERIC="1"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    twin = np.load(out)
    for name in CASES:
        g = util.load(f"matchpyramid_{name}.npz")
        got = _features(torch.tensor(g["q"]), torch.tensor(g["d"]), MR.params_from_golden(g), dev).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), twin[name].view(np.uint32)), name


# (n_queries, pairs_per_query, B, Q, D, E, channels, kernels, pools)
SWEEP = [
    (3, 1, 3, 30, 200, 300, *MR.DEFAULT),                                                    # E = 300, default pyramid
    (1, 1, 1, 64, 2048, 8, [4, 3], [[3, 3], [2, 2]], [[64, 256], [2, 3]]),                   # Q, D, pool at the limits
    (2, 1, 2, 6, 10, 16, [32] * 8, [[3, 3]] * 8, [[6, 10]] * 7 + [[2, 3]]),                  # 8 layers of 32 channels
    (2, 1, 2, 9, 23, 16, [6, 7], [[5, 5], [5, 5]], [[5, 11], [3, 4]]),                       # 5 x 5 kernels
    (2, 1, 2, 1, 1, 16, [3, 2], [[1, 1], [3, 3]], [[2, 2], [1, 1]]),                         # Q = 1, D = 1
    (2, 1, 2, 20, 300, 16, [3], [[3, 3]], [[1, 1]]),                                         # one window wider than a tile
    (1, 1000, 1000, 8, 20, 16, [4, 4], [[3, 3], [3, 3]], [[4, 8], [2, 3]]),                  # one shared query
    (3, 60, 130, 8, 20, 16, [4, 4], [[3, 3], [3, 3]], [[4, 8], [2, 3]]),                     # last group partial
]


@pytest.mark.parametrize("nq, ppq, B, Q, D, E, channels, kernels, pools", SWEEP)
def test_random_sweep_against_fp64(nq, ppq, B, Q, D, E, channels, kernels, pools):
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(Q * 7 + D + E + B)
    q = torch.randn(nq, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    d[:, ::13] = 0
    p = MR.random_params(channels, kernels, pools, seed=Q + D, scale=2.0)
    got = _features(q, d, p, dev, ppq)
    _check(got, q, d, p, f"sweep Q{Q} D{D} E{E} L{len(channels)}", ppq)


def test_two_calls_layouts_and_a_pair_alone_are_bit_equal():
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(5)
    q = torch.randn(2, 30, 64, generator=g)
    d = torch.randn(120, 200, 64, generator=g)
    p = MR.random_params(*MR.DEFAULT, seed=6, scale=2.0)
    a = _features(q, d, p, dev, 60)
    assert torch.equal(a, _features(q, d, p, dev, 60))                                          # two calls
    assert torch.equal(a, _features(q.repeat_interleave(60, dim=0), d, p, dev, 1))              # replicated query
    assert torch.equal(a[77:78], _features(q[1:2], d[77:78], p, dev, 1))                        # a pair alone
    w, b = MR.conv_lists(p)
    flat = [x for pool in p["pools"] for x in pool]
    t = torch.ops.mm_native.matchpyramid_features(q.to(dev), d.to(dev), [x.to(dev) for x in w], [x.to(dev) for x in b], flat, 60)
    assert torch.equal(a, t)
    with torch.autocast("cuda", dtype=torch.float16):                                           # inputs stay fp32
        t = torch.ops.mm_native.matchpyramid_features(q.to(dev), d.to(dev), [x.to(dev) for x in w], [x.to(dev) for x in b],
                                                      flat, 60)
    assert torch.equal(a, t)


# one step past every limit: (Q, D, E, channels, kernels, pools)
REFUSED = [
    (65, 20, 16, [4], [[3, 3]], [[2, 2]]),
    (8, 2049, 16, [4], [[3, 3]], [[2, 2]]),
    (8, 20, 1028, [4], [[3, 3]], [[2, 2]]),
    (8, 20, 16, [4] * 9, [[3, 3]] * 9, [[2, 2]] * 9),
    (8, 20, 16, [33], [[3, 3]], [[2, 2]]),
    (8, 20, 16, [4], [[6, 3]], [[2, 2]]),
    (8, 20, 16, [4], [[3, 6]], [[2, 2]]),
    (8, 20, 16, [4], [[3, 3]], [[65, 2]]),
    (8, 20, 16, [4], [[3, 3]], [[2, 257]]),
    (2, 20, 16, [4], [[5, 1]], [[2, 2]]),              # conv output of height 2 + 1 - 5 < 1
]


@pytest.mark.parametrize("Q, D, E, channels, kernels, pools", REFUSED)
def test_one_past_each_limit_is_refused_and_the_module_falls_back(Q, D, E, channels, kernels, pools):
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(Q + D)
    q, d = torch.randn(2, Q, E, generator=g), torch.randn(2, D, E, generator=g)
    p = MR.random_params(channels, kernels, pools, seed=3)
    with pytest.raises(NativeError) as e:
        _features(q, d, p, dev)
    assert e.value.code == _lib.MM_EUNSUPPORTED
    # the C entry point refuses the same shape itself, before any launch (the pointers are never dereferenced)
    import ctypes
    L = len(channels)
    rows = [x for c, k, pl in zip(channels, kernels, pools) for x in (c, k[0], k[1], pl[0], pl[1])]
    arr = (ctypes.c_int32 * (5 * L))(*rows)
    one = torch.zeros(4, device=dev)
    rc = _lib.lib().mm_matchpyramid_fwd(one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 2, 1, Q,
                                        D, E, L, arr, None, 0, None)
    assert rc == _lib.MM_EUNSUPPORTED
    assert _lib.lib().mm_matchpyramid_fwd(None, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 2, 1, 8, 20, 16,
                                          L, arr, None, 0, None) == _lib.MM_EINVAL
    if Q + kernels[0][1] - kernels[0][0] < 1:
        return                                           # the reference raises for this shape too
    from matchmaker_amd.matchpyramid import MatchPyramid
    m = MatchPyramid(channels, kernels, pools)
    m.load_state_dict({k: v for k, v in p.items() if k != "pools"}, strict=True)
    m = m.to(dev).eval()
    with torch.no_grad():
        s = m(q.to(dev), d.to(dev), None, None)
    s64 = MR.score(q, d, p, torch.float64)
    tol = MR.measured_tol(MR.score(q, d, p, torch.float32), s64)
    print(f"fallback: tol = {tol:.3e}")
    assert float((s.double().cpu() - s64).abs().max()) <= tol
    torch.cuda.synchronize()


def test_module_train_path_agrees_and_autocast_is_bit_equal():
    dev = util.require_gpu()
    g = util.load("matchpyramid_hot.npz")
    p = MR.params_from_golden(g)
    q, d = torch.tensor(g["q"]).to(dev), torch.tensor(g["d"]).to(dev)
    m = module_from_golden(g).to(dev)            # strict=True load inside
    m.eval()
    with torch.no_grad():
        s_native = m(q, d, None, None)
        with torch.autocast("cuda", dtype=torch.float16):
            f_auto = m.features(q, d)
        assert torch.equal(f_auto, m.features(q, d))
    m.train()
    assert all(x.requires_grad for x in m.parameters())
    s_train = m(q, d, None, None)
    assert s_train.requires_grad
    s64 = MR.score(q.cpu(), d.cpu(), p, torch.float64)
    tol = MR.measured_tol(MR.score(q.cpu(), d.cpu(), p, torch.float32), s64)
    print(f"train path: tol = {tol:.3e}")
    assert float((s_native.double().cpu() - s64).abs().max()) <= tol
    assert float((s_train.detach().double().cpu() - s64).abs().max()) <= tol
    s_train.sum().backward()
    for n, x in m.named_parameters():
        assert x.grad is not None and torch.isfinite(x.grad).all(), n


def test_rank_order_of_the_shared_list():
    dev = util.require_gpu()
    q, d, p = MR.rank_inputs()
    B = d.shape[0]
    s64 = MR.score(q, d, p, torch.float64, B)
    tol = MR.measured_tol(MR.score(q, d, p, torch.float32, B), s64)
    share = MR.undecided_share(s64, tol)
    print(f"rank order: tol = {tol:.3e}, undecided share = {share:.4f}")
    assert share <= 0.01
    got = MR.head(_features(q, d, p, dev, B).cpu(), p, torch.float64)
    assert float((got - s64).abs().max()) <= tol
    order = torch.argsort(s64, descending=True)
    a, b = s64[order], got[order]
    decided = (a[:-1] - a[1:]) > 2 * tol
    assert bool((b[:-1] > b[1:])[decided].all())


def test_graph_capture_replays_on_new_inputs():
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(9)
    p = MR.random_params(*MR.DEFAULT, seed=10, scale=2.0)
    w, b = MR.conv_lists(p)
    w, b = [t.to(dev) for t in w], [t.to(dev) for t in b]
    q, d = torch.randn(8, 30, 64, generator=g).to(dev), torch.randn(8, 200, 64, generator=g).to(dev)
    q2, d2 = torch.randn(8, 30, 64, generator=g).to(dev), torch.randn(8, 200, 64, generator=g).to(dev)
    ref2 = ops.matchpyramid_features(q2, d2, w, b, p["pools"])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.matchpyramid_features(q, d, w, b, p["pools"])
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # a host synchronisation inside would raise during capture
        out = ops.matchpyramid_features(q, d, w, b, p["pools"])
    q.copy_(q2)
    d.copy_(d2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref2)
