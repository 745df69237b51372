"""GPU tests of MatchPyramid's training path: mm_matchpyramid_fwd_save (the forward's bits plus every layer's pooled output and
arg-max), mm_matchpyramid_bwd, torch.ops.mm_native.matchpyramid_features_train and the module's native_backward switch.

Oracles, inputs, cases and the tolerance are tests/matchpyramid_bwd_reference.py's:
    tol = 4 max |g32 - g64| + max(16, sqrt(n)) 2^-24 max |g64|, g32 / g64 the same CPU oracle in fp32 / fp64, n from the shape.
The reference config's fp64 arg-max is not separated from fp32 noise (test_matchpyramid_bwd_cpu.py), so `ref` and `chan` are
compared with the given-arg-max oracle fed the kernel's own indices only, and the indices are validated on their own.
Every test prints its tolerances."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from matchmaker_amd import ops
from tests import matchpyramid_bwd_reference as BR
from tests import matchpyramid_reference as MR
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(BR.CASES)


def _on(dev, name):
    q, d, go, p = BR.inputs(name)
    w, b = MR.conv_lists(p)
    return q.to(dev), d.to(dev), go.to(dev), [t.to(dev) for t in w], [t.to(dev) for t in b], p["pools"]


def compute(name, dev, sel=None, ppq=1):
    """the save entry and the backward on a case (sel: a slice of the pairs) -> dict of CPU tensors"""
    q, d, go, w, b, pools = _on(dev, name)
    if sel is not None:
        q, d, go = q[sel].contiguous(), d[sel].contiguous(), go[sel].contiguous()
    f, saved = ops.matchpyramid_features_save(q, d, w, b, pools, ppq)
    gq, gd, gw, gb = ops.matchpyramid_bwd(q, d, w, b, pools, saved, go, ppq)
    torch.cuda.synchronize()
    return {"features": f.cpu(), "pooled": saved[0].cpu(), "argmax": saved[1].cpu(), "gq": gq.cpu(), "gd": gd.cpu(),
            "gw": [t.cpu() for t in gw], "gb": [t.cpu() for t in gb]}


@functools.lru_cache(maxsize=None)
def native(name):
    return compute(name, util.require_gpu())


def per_layer(name, flat):
    """[B, S] -> per layer [B, C, ph pw]"""
    out, o = [], 0
    for (C, _, _, _, _, _, _, _, ph, pw) in BR.geometry(name):
        out.append(flat[:, o:o + C * ph * pw].view(flat.shape[0], C, ph * pw))
        o += C * ph * pw
    assert o == flat.shape[1]
    return out


def _within(label, got, g32, g64, n):
    t = BR.tol(g32, g64, n)
    err = float((got.double() - g64.double()).abs().max()) if g64.numel() else 0.0
    print(f"{label}: n = {n}, tol = {t:.3e}, err = {err:.3e}, max |g64| = {float(g64.abs().max()) if g64.numel() else 0:.3e}")
    assert got.shape == g64.shape and torch.isfinite(got).all()
    assert err <= t, (label, err, t)


def _compare(name, got, o32, o64):
    per, emb = BR.sum_lengths(name)
    q, d, _, _ = BR.inputs(name)
    zq = q.abs().amax(-1) == 0                   # [B, Q] zero rows: their gradient is g / 1e-13, compared scaled by 1e-13
    zd = d.abs().amax(-1) == 0
    for key, z in (("gq", zq), ("gd", zd)):
        _within(f"{name} {key}", got[key][~z], o32[key][~z], o64[key][~z], emb)
        if bool(z.any()):
            _within(f"{name} {key} zero rows x 1e-13", got[key][z] * 1e-13, o32[key][z] * 1e-13, o64[key][z] * 1e-13, emb)
    for l, n in enumerate(per):
        _within(f"{name} grad_w[{l}]", got["gw"][l], o32["gw"][l], o64["gw"][l], n)
        _within(f"{name} grad_b[{l}]", got["gb"][l], o32["gb"][l], o64["gb"][l], n)


@pytest.mark.parametrize("name", ALL)
def test_save_entry_has_the_forwards_bits_and_the_last_pooled_is_features(name):
    dev = util.require_gpu()
    q, d, _, w, b, pools = _on(dev, name)
    got = native(name)
    assert torch.equal(got["features"], ops.matchpyramid_features(q, d, w, b, pools).cpu())
    last = per_layer(name, got["pooled"])[-1]
    assert torch.equal(last.reshape(last.shape[0], -1), got["features"])
    f64 = BR.oracle_a(name, torch.float64)["features"]
    t = MR.measured_tol(BR.oracle_a(name, torch.float32)["features"], f64)
    err = float((got["features"].double() - f64).abs().max())
    print(f"{name} features: tol = {t:.3e}, err = {err:.3e}")
    assert err <= t


@pytest.mark.parametrize("name", ALL)
def test_saved_argmax_is_valid(name):
    """inside its window; its fp64 value within 2 forward tol of the window's fp64 maximum; torch's own fp64 index wherever
    the element is decided (a positive maximum whose strict gap exceeds 2 tol), which on `zero` includes exact positive
    ties: the lowest flat index.  The pooled value is the fp64 maximum within tol."""
    got = native(name)
    t = BR.forward_tol(name)
    R64, idx64 = BR.planes(name, torch.float64)
    decided_n = tied_n = 0
    for l, (arg, pooled, geo) in enumerate(zip(per_layer(name, got["argmax"]), per_layer(name, got["pooled"]),
                                               BR.geometry(name))):
        C, _, _, _, _, _, Ho, Wo, ph, pw = geo
        arg = arg.long()
        assert int(arg.min()) >= 0 and int(arg.max()) < Ho * Wo
        row, col = (arg // Wo).view(-1, C, ph, pw), (arg % Wo).view(-1, C, ph, pw)
        rw, cw = torch.tensor(BR.windows(Ho, ph)), torch.tensor(BR.windows(Wo, pw))
        assert bool(((row >= rw[:, 0].view(1, 1, ph, 1)) & (row < rw[:, 1].view(1, 1, ph, 1))).all())
        assert bool(((col >= cw[:, 0].view(1, 1, 1, pw)) & (col < cw[:, 1].view(1, 1, 1, pw))).all())
        mx, gap, cnt = BR.element_gaps(name)[l]
        val = R64[l].flatten(2).gather(-1, arg).view_as(mx)
        assert bool((val >= mx - 2 * t).all()), (name, l, float((mx - val).max()), t)
        assert float((pooled.view_as(mx).double() - mx).abs().max()) <= t
        decided = (mx > 0) & (gap > 2 * t)
        decided_n += int(decided.sum())
        assert torch.equal(arg.view_as(mx)[decided], idx64[l].view_as(mx)[decided]), (name, l)
        tied = decided & (cnt > 1)
        tied_n += int(tied.sum())
    print(f"{name}: forward tol = {t:.3e}, decided elements = {decided_n}, of them exact ties = {tied_n}")
    assert decided_n > 0
    if name == "zero":
        assert tied_n > 0


@pytest.mark.parametrize("name", BR.DIRECT)
def test_gradients_against_the_modules_own_backward(name):
    _compare(name, native(name), BR.oracle_a(name, torch.float32), BR.oracle_a(name, torch.float64))


@pytest.mark.parametrize("name", ALL)
def test_gradients_against_the_given_argmax_form_fed_the_kernels_indices(name):
    got = native(name)
    arg = [a.long() for a in per_layer(name, got["argmax"])]
    _compare(name, got, BR.oracle_b(name, torch.float32, arg), BR.oracle_b(name, torch.float64, arg))


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("features", "pooled", "argmax", "gq", "gd")) and all(
        torch.equal(x, y) for x, y in zip(a["gw"] + a["gb"], b["gw"] + b["gb"]))


@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_two_calls_and_a_pair_alone_are_bit_equal(name):
    dev = util.require_gpu()
    a = native(name)
    assert _same(a, compute(name, dev))
    k = BR.CASES[name][0] - 1
    one = compute(name, dev, slice(k, k + 1))
    for key in ("features", "pooled", "argmax", "gq", "gd"):
        assert torch.equal(one[key][0], a[key][k]), key


def test_shared_queries_equal_the_replicated_call_summed():
    dev = util.require_gpu()
    q, d, go, w, b, pools = _on(dev, "tiny")
    q2 = q[:2].contiguous()                      # pairs 0, 1 -> query 0; pair 2 -> query 1 (the last group is partial)
    f, saved = ops.matchpyramid_features_save(q2, d, w, b, pools, 2)
    gq, gd, gw, gb = ops.matchpyramid_bwd(q2, d, w, b, pools, saved, go, 2)
    qr = q2.repeat_interleave(2, dim=0)[:3].contiguous()
    fr, savedr = ops.matchpyramid_features_save(qr, d, w, b, pools, 1)
    gqr, gdr, gwr, gbr = ops.matchpyramid_bwd(qr, d, w, b, pools, savedr, go, 1)
    assert torch.equal(f, fr) and torch.equal(saved[0], savedr[0]) and torch.equal(saved[1], savedr[1])
    assert torch.equal(gd, gdr) and all(torch.equal(x, y) for x, y in zip(gw + gb, gwr + gbr))
    per = gqr.cpu()
    s64 = torch.stack([per[:2].double().sum(0), per[2].double()])
    s32 = torch.stack([per[:2].sum(0), per[2]])
    assert tuple(gq.shape) == (2, 5, 8)
    _within("tiny grad_q, pairs_per_query = 2", gq.cpu(), s32, s64, 2)


def test_generic_twin_is_bit_equal_at_the_reference_config(tmp_path):
    """MM_MP_GENERIC is read once per process: the generic kernel runs in ONE fresh child"""
    util.require_gpu()
    out = tmp_path / "generic.npz"
    code = ("import sys, numpy as np, torch\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from tests.test_matchpyramid_bwd_gpu import compute\n"
            "r = compute('ref', torch.device('cuda:0'))\n"
            "flat = {k: v.numpy() for k, v in r.items() if not isinstance(v, list)}\n"
            "for k in ('gw', 'gb'):\n"
            "    flat.update({f'{k}{i}': t.numpy() for i, t in enumerate(r[k])})\n"
            f"np.savez({str(out)!r}, **flat)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MM_MP_GENERIC="1"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    twin, a = np.load(out), native("ref")
    for k in ("features", "pooled", "argmax", "gq", "gd"):
        assert np.array_equal(a[k].numpy().view(np.uint32), twin[k].view(np.uint32)), k
    for k in ("gw", "gb"):
        for i, t in enumerate(a[k]):
            assert np.array_equal(t.numpy().view(np.uint32), twin[f"{k}{i}"].view(np.uint32)), (k, i)


def _module_grads(m, q, d, coef):
    m.zero_grad(set_to_none=True)
    q = q.detach().clone().requires_grad_(True)
    (m(q, d, None, None) * coef).sum().backward()
    return {**{n: p.grad.detach().cpu() for n, p in m.named_parameters()}, "q": q.grad.detach().cpu()}


def test_module_trains_through_the_native_backward():
    dev = util.require_gpu()
    q, d, _, _ = BR.inputs("tiny")
    coef = torch.tensor([1.0, -2.0, 0.5])
    o32 = _module_grads(BR.module("tiny", torch.float32).train(), q, d, coef)
    o64 = _module_grads(BR.module("tiny", torch.float64).train(), q.double(), d.double(), coef.double())
    m = BR.module("tiny", torch.float32).to(dev).train()
    m.native_backward = False
    eager = _module_grads(m, q.to(dev), d.to(dev), coef.to(dev))
    m.native_backward = True
    seen = []
    orig = ops.matchpyramid_bwd
    try:
        ops.matchpyramid_bwd = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
        got = _module_grads(m, q.to(dev), d.to(dev), coef.to(dev))
    finally:
        ops.matchpyramid_bwd = orig
    assert seen, "the native backward did not run"
    n = max(BR.sum_lengths("tiny")[0])
    assert set(got) == set(eager) and any(k.startswith("dense") for k in got)
    for k in sorted(got):
        t = BR.tol(o32[k], o64[k], n)
        err = float((got[k].double() - eager[k].double()).abs().max())
        print(f"module {k}: n = {n}, tol = {t:.3e}, native - eager = {err:.3e}")
        assert err <= t, (k, err, t)
        assert float((got[k].double() - o64[k]).abs().max()) <= t, k
    with torch.no_grad():                        # the inference path is unchanged by the switch
        assert torch.equal(m.features(q.to(dev), d.to(dev)), native("tiny")["features"].to(dev))


def test_wrong_saved_state_and_grad_shapes_are_refused_before_any_launch():
    """these checks are what keeps the kernel from reading past pooled / argmax / grad_features"""
    from matchmaker_amd import NativeError
    dev = util.require_gpu()
    q, d, go, w, b, pools = _on(dev, "tiny")
    f, (pooled, argmax) = ops.matchpyramid_features_save(q, d, w, b, pools)
    B, S = pooled.shape
    bad = [
        ((pooled[:, :-1].contiguous(), argmax), go, "saved must be"),                     # a short row
        ((pooled, argmax[:, :-1].contiguous()), go, "saved must be"),
        ((pooled[:-1].contiguous(), argmax[:-1].contiguous()), go, "saved must be"),      # a pair missing
        ((pooled, argmax.long()), go, "saved must be"),                                   # int64 indices
        ((pooled.double(), argmax), go, "saved must be"),
        ((pooled, argmax), go[:, :-1].contiguous(), "grad_features must be"),             # a narrow gradient
        ((pooled, argmax), go[:-1].contiguous(), "grad_features must be"),
    ]
    for saved, g, msg in bad:
        with pytest.raises(NativeError, match=msg):
            ops.matchpyramid_bwd(q, d, w, b, pools, saved, g)
    with pytest.raises(NativeError, match="pool sizes"):
        ops.matchpyramid_bwd(q, d, w, b, pools[:1], (pooled, argmax), go)
    with pytest.raises(NativeError, match="pool sizes"):
        ops.matchpyramid_features_save(q, d, w, b, pools[:1])
    with pytest.raises(NativeError, match="biases"):
        ops.matchpyramid_bwd(q, d, w, b[:1], pools, (pooled, argmax), go)
    with pytest.raises(NativeError):                                                      # q of another batch size
        ops.matchpyramid_bwd(q[:-1].contiguous(), d, w, b, pools, (pooled, argmax), go)
    torch.cuda.synchronize()
    assert _same(native("tiny"), compute("tiny", dev))                                    # and the good call still works


def test_double_backward_raises():
    dev = util.require_gpu()
    q, d, go, w, b, pools = _on(dev, "tiny")
    q = q.clone().requires_grad_(True)
    flat = [x for p in pools for x in p]
    f = torch.ops.mm_native.matchpyramid_features_train(q, d, w, b, flat, 1)[0]
    (gq,) = torch.autograd.grad((f * go).sum(), q, create_graph=True)
    assert torch.equal(gq.detach().cpu(), native("tiny")["gq"])
    with pytest.raises(RuntimeError):
        gq.sum().backward()


def test_graph_capture_replays_on_new_inputs():
    dev = util.require_gpu()
    q2, d2, go2, w, b, pools = _on(dev, "ref")
    g = torch.Generator().manual_seed(9)
    q, d, go = (torch.randn(t.shape, generator=g).to(dev) for t in (q2, d2, go2))

    def step():
        f, saved = ops.matchpyramid_features_save(q, d, w, b, pools)
        return (f,) + ops.matchpyramid_bwd(q, d, w, b, pools, saved, go)

    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # a host synchronisation inside would raise during capture
        f, gq, gd, gw, gb = step()
    q.copy_(q2)
    d.copy_(d2)
    go.copy_(go2)
    graph.replay()
    torch.cuda.synchronize()
    a = native("ref")
    assert torch.equal(f.cpu(), a["features"]) and torch.equal(gq.cpu(), a["gq"]) and torch.equal(gd.cpu(), a["gd"])
    assert all(torch.equal(x.cpu(), y) for x, y in zip(gw + gb, a["gw"] + a["gb"]))
