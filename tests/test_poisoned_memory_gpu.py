"""GPU: every operator of matchmaker_amd/ops.py writes all it owns and no more (tests/poison.py; the audit table is there).

Each case runs one operator twice on one small, edge-bearing input — its outputs and workspaces carved from memory filled
with 0xFF, then with 0x7F — and asserts that (1) every guard byte around every allocation, workspaces included, is intact,
(2) the two results are bit-identical over every element include/mm_native.h specifies, and (3) the result meets the
operator's existing reference at the tolerance of that operator's existing test (named in each case; no new number).

Excluded from (2): only `pooled` of mm_kernel_pool_ex_fwd2, "Rows of padded / masked query tokens are unspecified"
(include/mm_native.h) — exactly the rows the query mask removes, under half of the tensor (asserted).

Atomics (read in csrc/): dot_topk.hip, dot_topk_fp8.hip, ivf_device.h and graph_search.hip use atomicAdd / atomicMax /
atomicMin / atomicCAS on int32 counters, histogram bins, slot numbers and the visited table only — never on a float.  The
slot a candidate lands in varies from run to run, the sorted output does not (equal scores: lower row first), so these
operators are held to the bit comparison like every other; none needed the tolerance fallback.

Chains run the producer under both poisons, check on the host that every integer hand-off tensor is identical across the two
runs and in range (else: fail, nothing more is launched), then run the consumer under poison on each producer run's own
outputs; unspecified float parts stay poisoned.

test_pooling_backward_twins_*: the kernels and launch forms of the pooling backward that only an environment switch selects
(common.hip reads it once per process), one fresh child process per setting."""
import functools
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import np_oracle as O
from oracle import torch_port as TP
from tests import poison, util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU = [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9]
SIGMA = [0.1] * 11

# name, the public operators of ops.py the case runs under poison, build(dev) -> stage
Case = namedtuple("Case", "name ops build")
CASES = []

# operators that reach native code and have no case, with the reason
WAIVERS = {
    "hbm_stream_probe": "a calibration launch that only reads its input: no output, no workspace, nothing to poison",
}


def case(name, *ops_):
    def deco(fn):
        CASES.append(Case(name, ops_, fn))
        return fn
    return deco


# A stage is a dict:
#   run()            the operator call(s), made under poison                     -> result (tensors, nested tuples / lists)
#   check(result)    the comparison with the operator's reference at its existing tolerance
#   keep(result)     optional: per output tensor a bool mask of the specified elements (None: all)
#   ints(result)     optional, chains: [(name, tensor, lo, hi)] integer hand-offs, all values in [lo, hi)
#   next(result)     optional, chains: the consumer stages for this producer result
def _drive(stages, label):
    outs = [poison.run(st["run"], p, label=f"{label} [{p:#04x}]")[0] for st, p in zip(stages, poison.POISONS)]
    keep = stages[0]["keep"](outs[0]) if "keep" in stages[0] else None
    if keep is not None:
        for t, m in zip(poison.flatten(outs[0]), keep):
            if m is not None:
                share = 1.0 - float(m.expand_as(t).float().mean())
                assert share < 0.5, f"{label}: {share:.2f} of an output is excluded from the comparison"
    poison.assert_same_bits(outs[0], outs[1], label, keep)
    stages[0]["check"](outs[0])
    if "next" not in stages[0]:
        return
    for (name, a, lo, hi), (_, b, _, _) in zip(stages[0]["ints"](outs[0]), stages[1]["ints"](outs[1])):
        assert torch.equal(a, b), f"{label}: hand-off {name} differs between the two producer runs; consumer not launched"
        if a.numel():
            assert lo <= int(a.min()) and int(a.max()) < hi, \
                f"{label}: hand-off {name} leaves [{lo}, {hi}): [{int(a.min())}, {int(a.max())}]; consumer not launched"
    consumers = [st["next"](o) for st, o in zip(stages, outs)]
    for i in range(len(consumers[0])):
        _drive([consumers[0][i], consumers[1][i]], f"{label} -> {consumers[0][i]['name']}")


def _np(t):
    return t.detach().cpu().numpy()


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _equal(got, ref, label):
    np.testing.assert_array_equal(_np(got[0]).astype(np.float64), ref[0], err_msg=f"{label}: scores")
    np.testing.assert_array_equal(_np(got[1]), ref[1], err_msg=f"{label}: rows")


# ======================================================================================================= MaxSim
def _maxsim_inputs(dtype, Q, D, E, seed):
    """3 queries x 3 pairs, the last group one short (B = 8); q lengths Q / 5 / 1; a full, an empty (fully masked) and ragged
    documents, one with a hole; dense int64 masks (the mask-packing workspace is used)."""
    g = torch.Generator().manual_seed(seed)
    nq, ppq, B = 3, 3, 8
    q = (torch.randn(nq, Q, E, generator=g) * 0.25).to(dtype)
    d = (torch.randn(B, D, E, generator=g) * 0.25).to(dtype)
    q_len = torch.tensor([Q, 5, 1])
    d_len = torch.randint(1, D + 1, (B,), generator=g)
    d_len[0], d_len[3], d_len[-1] = D, 0, D // 2 + 1
    qm = (torch.arange(Q)[None] < q_len[:, None]).long()
    dm = (torch.arange(D)[None] < d_len[:, None]).long()
    dm[0, D // 3] = 0
    return q, d, qm, dm, ppq


def _maxsim_case(dtype, tol, Q, D, E):
    def build(dev):
        from matchmaker_amd import ops
        q, d, qm, dm, ppq = _maxsim_inputs(dtype, Q, D, E, Q * 1000 + D)
        a = [t.to(dev) for t in (q, d, qm, dm)]
        qi = np.arange(d.shape[0]) // ppq
        ref = O.maxsim_paired(q.float().numpy()[qi], d.float().numpy(), qm.numpy()[qi], dm.numpy())

        def check(out):      # tests/test_maxsim_gpu.py::test_shared_query_layout_random
            np.testing.assert_allclose(_np(out), ref, atol=tol, rtol=1e-4)
        return {"run": lambda: ops.maxsim(*a, pairs_per_query=ppq), "check": check}
    return build


for _dt, _tol, _Q, _D, _E in [(torch.bfloat16, util.TOL_BF16, 32, 180, 128), (torch.float32, util.TOL_FP32, 13, 47, 24),
                              (torch.bfloat16, util.TOL_BF16, 13, 47, 24), (torch.float32, util.TOL_FP32, 32, 180, 128)]:
    case(f"maxsim-{str(_dt)[6:]}-Q{_Q}-D{_D}-E{_E}", "maxsim")(_maxsim_case(_dt, _tol, _Q, _D, _E))


@case("maxsim_batched-3-batches-bf16-Q32-D180-E128", "maxsim_batched")
def _maxsim_batched(dev):
    """Three pair-per-row batches of 5 / 1 / 3 pairs in one launch: int64 tokenizer masks, a hole, a fully padded document."""
    from matchmaker_amd import ops
    g = torch.Generator().manual_seed(32128)
    Q, D, E = 32, 180, 128
    batches, refs = [], []
    for B in (5, 1, 3):
        q = (torch.randn(B, Q, E, generator=g) / E ** 0.5).to(torch.bfloat16)
        d = (torch.randn(B, D, E, generator=g) / E ** 0.5).to(torch.bfloat16)
        qm = (torch.arange(Q)[None] < torch.randint(1, Q + 1, (B, 1), generator=g)).long()
        dm = (torch.arange(D)[None] < torch.randint(1, D + 1, (B, 1), generator=g)).long()
        dm[0, 3] = 0
        dm[-1] = 0 if B == 3 else dm[-1]
        batches.append(tuple(t.to(dev) for t in (q, d, qm, dm)))
        refs.append(O.maxsim_paired(q.float().numpy(), d.float().numpy(), qm.numpy(), dm.numpy()))

    def check(out):          # tests/test_maxsim_gpu.py::test_forward_matches_reference_golden (bf16)
        for s, ref in zip(out, refs):
            np.testing.assert_allclose(_np(s), ref, atol=util.TOL_BF16, rtol=1e-4)
    return {"run": lambda: ops.maxsim_batched(batches), "check": check}


def _ragged_store(rng, n_docs, E, dtype, max_len, empty):
    lens = rng.integers(1, max_len + 1, n_docs)
    lens[list(empty)] = 0
    end = np.cumsum(lens)
    tok = torch.from_numpy(rng.standard_normal((int(end[-1]), E)).astype(np.float32)).to(dtype)
    return tok, (end - lens).astype(np.int64), end.astype(np.int64)


def _ragged_ref(q, q_len, tok, begin, end, ppq):
    qf, tf = q.float(), tok.float()
    out = np.zeros(len(begin))
    for p, (b, e) in enumerate(zip(begin, end)):
        i = p // ppq
        n = int(q_len[i])
        out[p] = float((qf[i, :n] @ tf[b:e].T).max(-1).values.sum()) if e > b else -1000.0 * n      # (an empty range: colbert.py:69)
    return out


def _ragged_case(dtype, tol, Q, E):
    def build(dev):
        from matchmaker_amd import ops
        rng = np.random.default_rng(E + Q)
        tok, begin, end = _ragged_store(rng, 12, E, dtype, 70, empty=(4,))
        nq, ppq, B = 2, 5, 9
        q = torch.from_numpy(rng.standard_normal((nq, Q, E)).astype(np.float32) / np.sqrt(E)).to(dtype)
        cand = rng.integers(0, 12, B)
        cand[0], cand[3] = 11, 4                  # the last document of the store; the empty one
        q_len = torch.tensor([Q, 7], dtype=torch.int32)
        a = (q.to(dev), tok.to(dev), _t(begin[cand], dev), _t(end[cand], dev), q_len.to(dev))
        ref = _ragged_ref(q, q_len, tok, begin[cand], end[cand], ppq)

        def check(out):      # tests/test_maxsim_ragged_bwd_gpu.py::test_ragged_matches_per_document_aggregation
            assert (np.abs(_np(out) - ref) <= tol + 1e-4 * np.abs(ref)).all(), (_np(out), ref)
        return {"run": lambda: ops.maxsim_ragged(*a, pairs_per_query=ppq), "check": check}
    return build


case("maxsim_ragged-bf16-Q32-E128", "maxsim_ragged")(_ragged_case(torch.bfloat16, util.TOL_BF16, 32, 128))
case("maxsim_ragged-f32-Q13-E24", "maxsim_ragged")(_ragged_case(torch.float32, util.TOL_FP32, 13, 24))


def _ragged_fp8_case(Q, E):
    def build(dev):
        from matchmaker_amd import ops
        from tests import fp8_store_reference as R
        c = R.exact_case(Q, E, 7, seed=1000 * Q + E + 7)          # document lengths 0 .. 200, a short last query, a mask with a hole
        q = _t(c["q"], dev, torch.bfloat16)
        a = (q, _t(c["codes"], dev), _t(c["scales"], dev), _t(c["begin"], dev), _t(c["end"], dev), _t(c["mask"], dev))
        ref = R.maxsim_ragged_fp8_ref(c["q"], c["codes"], c["scales"], c["begin"], c["end"], q_mask=c["mask"], pairs_per_query=7,
                                      q_dtype=torch.bfloat16)

        def check(out):      # tests/test_fp8_store_gpu.py::test_maxsim_is_bit_equal_on_exactly_representable_data
            assert np.array_equal(_np(out).astype(np.float64), ref)
        return {"run": lambda: ops.maxsim_ragged_fp8(*a, pairs_per_query=7), "check": check}
    return build


case("maxsim_ragged_fp8-Q33-E128", "maxsim_ragged_fp8")(_ragged_fp8_case(33, 128))
case("maxsim_ragged_fp8-Q13-E48", "maxsim_ragged_fp8")(_ragged_fp8_case(13, 48))


def _quantize_case(T, E, dtype):
    def build(dev):
        from matchmaker_amd import ops
        from tests import fp8_store_reference as R
        x = R.special_rows(T, E, dtype, seed=100 + E)
        want_c, want_s = R.quantize_torch(x)
        xd = x.to(dev)

        def check(out):      # tests/test_fp8_store_gpu.py::test_quantiser_is_bit_equal_to_the_restatement
            assert torch.equal(out[1].cpu(), want_s) and torch.equal(R.fold_zero(out[0].cpu()), R.fold_zero(want_c))
        return {"run": lambda: ops.fp8_quantize_rows(xd), "check": check}
    return build


case("fp8_quantize_rows-f16-T33-E128", "fp8_quantize_rows")(_quantize_case(33, 128, torch.float16))
case("fp8_quantize_rows-f32-T1-E16", "fp8_quantize_rows")(_quantize_case(1, 16, torch.float32))


def _maxsim_bwd_case(dtype, tol, B, Q, D, E, grad_dtype=None):
    def build(dev):
        from matchmaker_amd import ops
        g = torch.Generator().manual_seed(B * 1000 + D)
        q = (torch.randn(B, Q, E, generator=g) / E ** 0.5).to(dtype)
        d = torch.randn(B, D, E, generator=g).to(dtype)
        q_len = torch.randint(1, Q + 1, (B,), generator=g)
        d_len = torch.randint(1, D + 1, (B,), generator=g)
        q_len[0], q_len[2], d_len[0], d_len[-1] = Q, 1, D, 0      # a fully padded document: no gradient at all
        qm = (torch.arange(Q)[None] < q_len[:, None]).long()
        dm = (torch.arange(D)[None] < d_len[:, None]).long()
        dm[1, 0] = 0
        go = torch.randn(B, generator=g)
        _, ref_gq, ref_gd = TP.maxsim_forward_backward(q, d, qm, dm, go)
        a = [t.to(dev) for t in (q, d, qm, dm, go)]

        def check(out):      # tests/test_maxsim_ragged_bwd_gpu.py::test_backward_matches_autograd_of_the_reference_ops
            gq, gd = out
            assert gq.shape == q.shape and gd.shape == d.shape
            if grad_dtype is None:
                kw = dict(atol=tol, rtol=1e-5)
            else:            # (the 16-bit gradients of the same test, through the drop-in)
                assert gq.dtype == dtype and gd.dtype == dtype
                kw = dict(atol=max(tol, 2e-2), rtol=1e-2)
            np.testing.assert_allclose(_np(gq.float()), ref_gq.numpy(), **kw)
            np.testing.assert_allclose(_np(gd.float()), ref_gd.numpy(), **kw)
            assert float(gd[-1].float().abs().max()) == 0.0 and float(gq[-1].float().abs().max()) == 0.0
        return {"run": lambda: ops.maxsim_bwd(*a, grad_dtype=grad_dtype), "check": check}
    return build


case("maxsim_bwd-f32-Q13-D47-E24", "maxsim_bwd")(_maxsim_bwd_case(torch.float32, 1e-4, 5, 13, 47, 24))
case("maxsim_bwd-bf16-Q32-D180-E128", "maxsim_bwd")(_maxsim_bwd_case(torch.bfloat16, 1e-2, 4, 32, 180, 128))
case("maxsim_bwd-bf16-grads-bf16-Q13-D47-E24", "maxsim_bwd")(_maxsim_bwd_case(torch.bfloat16, 1e-2, 5, 13, 47, 24, torch.bfloat16))
case("maxsim_bwd-f32-Q32-D180-E128", "maxsim_bwd")(_maxsim_bwd_case(torch.float32, 1e-4, 4, 32, 180, 128))


# all-pairs MaxSim: the exact-arithmetic inputs of tests/test_maxsim_inbatch_bwd_gpu.py (multiples of 1/8; a padded tail, mask
# holes, a fully padded document, a padded query tail; Bq != Bd)
INBATCH = [((3, 5, 13, 47, 64), torch.float32, False), ((2, 9, 32, 180, 128), torch.bfloat16, False),
           ((4, 4, 40, 70, 24), torch.bfloat16, True), ((4, 4, 40, 70, 24), torch.float32, False)]


def _inbatch_case(shape, dt, bug):
    def build(dev):
        from matchmaker_amd import ops
        from tests.test_maxsim_inbatch_bwd_gpu import _exact_case
        q, qm, d, dm, _, _, _ = _exact_case(*shape, bug)
        a = (q.to(dev, dt), qm.to(dev), d.to(dev, dt), dm.to(dev))
        ref = O.maxsim_inbatch(q.numpy(), qm.numpy(), d.numpy(), dm.numpy(), bug_compatible=bug)
        tol = util.TOL_FP32 if dt == torch.float32 else util.TOL_BF16

        def check(out):      # tests/test_maxsim_gpu.py::test_inbatch_matches_reference_golden
            np.testing.assert_allclose(_np(out), ref, atol=tol, rtol=1e-4)
        return {"run": lambda: ops.maxsim_inbatch(*a, bug_compatible=bug), "check": check}
    return build


def _inbatch_bwd_case(shape, dt, bug):
    def build(dev):
        from matchmaker_amd import ops
        from tests.test_maxsim_inbatch_bwd_gpu import _assert_bits, _exact_case
        q, qm, d, dm, go, ref, _ = _exact_case(*shape, bug)
        a = (q.to(dev, dt), qm.to(dev), d.to(dev, dt), dm.to(dev), go.to(dev))

        def check(out):      # tests/test_maxsim_inbatch_bwd_gpu.py::test_exact_arithmetic_inputs_are_bit_equal_to_the_restatement
            assert out[0].shape == q.shape and out[1].shape == d.shape and out[0].dtype == dt
            _assert_bits(out[0], ref["gq"], "grad_q")
            _assert_bits(out[1], ref["gd"], "grad_d")
        return {"run": lambda: ops.maxsim_inbatch_bwd(*a, bug_compatible=bug, grad_dtype=dt), "check": check}
    return build


for _shape, _dt, _bug in INBATCH:
    _id = "x".join(map(str, _shape)) + "-" + str(_dt)[6:] + ("-bug" if _bug else "")
    case("maxsim_inbatch-" + _id, "maxsim_inbatch")(_inbatch_case(_shape, _dt, _bug))
    case("maxsim_inbatch_bwd-" + _id, "maxsim_inbatch_bwd")(_inbatch_bwd_case(_shape, _dt, _bug))


# ======================================================================================================= kernel pooling
def pool_inputs(B, Q, D, E, K, gated, seed):
    """Pair-per-row pooling inputs with every mask edge: query lengths Q / 7 / 1 (cycled), document lengths D / 0 / 33 (or
    D // 2) / D - 1 (cycled), a hole in document 0's mask, planted near matches, a gate that closes about half of the tokens."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    for b in range(B):
        d[b, b % D] = q[b, b % Q] * 1.3 + 0.05 * torch.randn(E, generator=g)
    q_len = torch.tensor([[Q, min(7, Q), 1, Q][b % 4] for b in range(B)])
    d_len = torch.tensor([[D, 0, min(33, D // 2), D - 1][b % 4] for b in range(B)])
    qm = (torch.arange(Q)[None] < q_len[:, None]).float()
    dm = (torch.arange(D)[None] < d_len[:, None]).float()
    if D > 2:
        dm[0, 1] = 0.0
    mu = torch.tensor(MU) if K == 11 else torch.linspace(1.0, -0.9, K)
    sigma = torch.full((K,), 0.1)
    alpha = torch.rand(K, generator=g) + 0.5
    w = torch.randn(K, generator=g) * 0.3
    go = torch.randn(B, generator=g)
    gate = None
    if gated:
        gate = torch.relu(torch.randn(B, D, generator=g)) * dm
        for b in range(B):
            gate[b, b % D] = 0.8 * dm[b, b % D]
    return dict(q=q, d=d, qm=qm, dm=dm, mu=mu, sigma=sigma, alpha=alpha, w=w, go=go, gate=gate, K=K)


def pool_fwd_reference(x):
    q, d, qm, dm = (x[k].numpy() for k in ("q", "d", "qm", "dm"))
    p = [x[k].numpy() for k in ("mu", "sigma", "alpha", "w")]
    if x["gate"] is None:
        return O.tk_kernel_pool(q, d, qm, dm, *p, dtype=np.float64, return_per_kernel=True)
    return O.tk_sparse_kernel_pool(q, d, qm, dm, x["gate"].numpy(), *p, dtype=np.float64, return_per_kernel=True)


def pool_bwd_reference(x):
    """fp64 autograd through the torch port: [grad_q, grad_d, grad_alpha, grad_w(, grad_gate)] as numpy"""
    dt = torch.float64
    names = ("q", "d", "alpha", "w") + (("gate",) if x["gate"] is not None else ())
    leaves = [x[k].detach().to(dt).clone().requires_grad_(True) for k in names]
    mu, sigma = x["mu"].to(dt).view(1, 1, 1, -1), x["sigma"].to(dt).view(1, 1, 1, -1)
    if x["gate"] is None:
        s = TP.tk_kernel_pool(leaves[0], leaves[1], x["qm"].to(dt), x["dm"].to(dt), mu, sigma, leaves[2].view(1, 1, -1), leaves[3].view(1, -1))
    else:
        s = TP.tk_sparse_kernel_pool(leaves[0], leaves[1], x["qm"].to(dt), x["dm"].to(dt), leaves[4].unsqueeze(1), mu, sigma,
                                     leaves[2].view(1, 1, -1), leaves[3].view(1, -1))
    s.backward(x["go"].to(dt))
    return [t.grad.numpy() for t in leaves]


def check_pool_bwd(got, want, label):
    """tests/test_kernel_pool_gpu.py::test_kernel_pool_backward_matches_autograd_of_the_reference_ops and
    tests/test_variants_gpu.py::test_gated_backward_matches_autograd_of_the_reference_ops: atol 2e-4 x scale, rtol 2e-3"""
    assert len(got) == len(want)
    for g_, w_, name in zip(got, want, ("grad_q", "grad_d", "grad_alpha", "grad_w", "grad_gate")):
        scale = max(1.0, float(np.abs(w_).max()))
        np.testing.assert_allclose(_np(g_).astype(np.float64), w_, atol=2e-4 * scale, rtol=2e-3, err_msg=f"{label} {name}")


def _pool_dev(x, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in x.items()}


def _pool_fwd_stage(x, xd, chain_to_bwd):
    from matchmaker_amd import ops
    K = x["K"]

    def run():
        return ops.kernel_pool(xd["q"], xd["d"], xd["qm"], xd["dm"], xd["mu"], xd["sigma"], xd["alpha"], xd["w"],
                               return_per_kernel=True, d_gate=xd["gate"], return_pooled=True)

    def check(out):          # tests/test_kernel_pool_gpu.py::test_kernel_pool_random, tests/test_variants_gpu.py::test_gated_kernel_pool_vs_oracle,
        s, pk, pooled = out  # ::test_kernel_counts_other_than_eleven (the K / 11 factor)
        ref, ref_pk = pool_fwd_reference(x)
        assert pooled.shape == (x["q"].shape[0], x["q"].shape[1], K)
        np.testing.assert_allclose(_np(pk), ref_pk, atol=5e-3, rtol=1e-4)
        np.testing.assert_allclose(_np(s), ref, atol=util.TOL_FP32 * max(1.0, K / 11), rtol=1e-5)

    st = {"run": run, "check": check, "keep": lambda out: [None, None, xd["qm"].bool().unsqueeze(-1)]}     # "Rows of padded / masked query tokens are unspecified"
    if chain_to_bwd:
        st["ints"] = lambda out: []
        st["next"] = lambda out: [_pool_bwd_stage(x, xd, out[2])]
    return st


def _pool_bwd_stage(x, xd, pooled=None):
    from matchmaker_amd import ops

    def run():
        return ops.kernel_pool_bwd(xd["q"], xd["d"], xd["qm"], xd["dm"], xd["mu"], xd["sigma"], xd["alpha"], xd["w"], xd["go"],
                                   d_gate=xd["gate"], pooled=pooled)

    def check(out):
        check_pool_bwd(out, pool_bwd_reference(x), "pooled path" if pooled is not None else "pre-pass path")
        qm, dm = xd["qm"].bool(), xd["dm"].bool()
        assert not out[0][~qm].any() and not out[1][~dm].any(), "masked rows carry gradient"
    return {"name": "kernel_pool_bwd", "run": run, "check": check}


# (B, Q, D, E, K): E = 300 and 64 take the split backward (Q <= 32, K = 11, E <= 320), E = 30 is padded to 32 by _pad_rows and
# trimmed again, E = 448 takes the tiled exact-f32 backward, Q = 33 the per-element backward, K = 5 the run-time-K kernels
POOL_SHAPES = [(4, 20, 70, 300, 11), (4, 20, 70, 64, 11), (4, 20, 70, 30, 11), (4, 20, 70, 448, 11), (4, 33, 70, 128, 11), (4, 20, 70, 64, 5)]


def _pool_case(shape, gated, what):
    def build(dev):
        x = pool_inputs(*shape, gated, seed=sum(shape) + gated)
        xd = _pool_dev(x, dev)
        if what == "fwd":
            return _pool_fwd_stage(x, xd, False)
        if what == "bwd":
            return _pool_bwd_stage(x, xd)
        return _pool_fwd_stage(x, xd, True)
    return build


for _shape in POOL_SHAPES:
    for _gated in (False, True):
        _id = "B{}-Q{}-D{}-E{}-K{}".format(*_shape) + ("-gated" if _gated else "")
        case("kernel_pool-" + _id, "kernel_pool")(_pool_case(_shape, _gated, "fwd"))
        case("kernel_pool_bwd-" + _id, "kernel_pool_bwd")(_pool_case(_shape, _gated, "bwd"))
for _shape in [POOL_SHAPES[0], POOL_SHAPES[2], POOL_SHAPES[3]]:
    for _gated in (False, True):
        _id = "B{}-Q{}-D{}-E{}-K{}".format(*_shape) + ("-gated" if _gated else "")
        case("chain-kernel_pool->kernel_pool_bwd-" + _id, "kernel_pool", "kernel_pool_bwd")(_pool_case(_shape, _gated, "chain"))


def _pool_multi_case(E, D):
    def build(dev):
        from matchmaker_amd import ops
        g = torch.Generator().manual_seed(E + D)
        B, Q, n = 5, 12, 2
        qs = [torch.relu(torch.randn(B, Q, E, generator=g)) for _ in range(n)]
        ds = [torch.relu(torch.randn(B, D, E, generator=g)) for _ in range(n)]
        qm = (torch.arange(Q)[None] < torch.tensor([Q, 7, 1, Q, 3])[:, None]).float()
        dm = (torch.arange(D)[None] < torch.tensor([D, 0, D // 2, D - 1, 1])[:, None]).float()
        ones = torch.ones(11)
        w = torch.randn(n * n, 11, generator=g) * 0.01
        ref = np.zeros(B)
        for i in range(n):
            for j in range(n):
                ref += O.tk_kernel_pool(qs[i].numpy(), ds[j].numpy(), qm.numpy(), dm.numpy(), MU, SIGMA, ones.numpy(),
                                        w[i * n + j].numpy(), dtype=np.float64)
        t = lambda v: v.to(dev)      # noqa: E731
        a = ([t(v) for v in qs], [t(v) for v in ds], t(qm), t(dm), t(torch.tensor(MU)), t(torch.tensor(SIGMA)), t(ones), t(w))

        def check(out):      # tests/test_kernel_pool_gpu.py::test_multi_block_pooling_equals_the_sum_of_single_launches
            np.testing.assert_allclose(_np(out), ref, atol=util.TOL_FP32, rtol=1e-5)
        return {"run": lambda: ops.kernel_pool_multi(*a), "check": check}
    return build


case("kernel_pool_multi-E64-D50", "kernel_pool_multi")(_pool_multi_case(64, 50))
case("kernel_pool_multi-E30-D33", "kernel_pool_multi")(_pool_multi_case(30, 33))


# ======================================================================================================= TKL
def _tkl_setup(dev, sat, D):
    """B = 3: a full document, an empty one (no chunk at all), one of a single chunk; Q = 7 with lengths 7 / 3 / 1, E = 64."""
    from matchmaker_amd.tkl import chunk_documents
    from tests.test_tkl_gpu import make_model
    B, Q, E = 3, 7, 64
    gen = torch.Generator().manual_seed(3000 + D)
    m = make_model(E, sat, dev).train()
    with torch.no_grad():      # off the init plateau, as tests/test_tkl_gpu.py's backward tests do
        for lin in (m.saturation_linear, m.saturation_linear2, m.saturation_linear3):
            lin.bias.fill_(2.0)
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * 0.3)
        for p in (m.chunk_scoring, m.kernel_mult, m.sat_normer.weight):
            p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
        m.sat_normer.bias.copy_(torch.rand(2, generator=gen) - 0.5)
    q = torch.randn(B, Q, E, generator=gen)
    d = torch.randn(B, D, E, generator=gen)
    for b in range(B):
        d[b, (7 * b) % D] = q[b, b % Q]
        d[b, (11 * b + 3) % D] = q[b, (b + 1) % Q] + 0.1 * torch.randn(E, generator=gen)
    qm = (torch.arange(Q)[None] < torch.tensor([Q, 3, 1])[:, None]).float()
    dm = (torch.arange(D)[None] < torch.tensor([D, 0, 33])[:, None]).float()
    qd, dd, qmd, dmd = q.to(dev), d.to(dev), qm.to(dev), dm.to(dev)
    q_ctx = qd * qmd.unsqueeze(-1)
    chunks, cmask, slot, C = chunk_documents(dd * dmd.unsqueeze(-1), dmd)
    assert int((slot // C == 1).sum()) == 0 and int((slot // C == 2).sum()) == 1
    return dict(m=m, q=q, d=d, qm=qm, dm=dm, q_ctx=q_ctx, chunks=chunks, cmask=cmask, slot=slot, C=C, qmd=qmd, B=B, sat=sat,
                go=torch.randn(B, generator=gen).to(dev))


def _tkl_fwd_stage(s, chain):
    from matchmaker_amd import ops
    m = s["m"]

    def run():
        return ops.tkl_score(s["q_ctx"], s["chunks"], s["cmask"], s["slot"], s["qmd"], m.pack_params(), s["B"], s["C"], 11, s["sat"],
                             return_peaks=True)

    def check(out):          # tests/test_tkl_gpu.py::test_tkl_random_vs_oracle
        score, win, peaks = out
        params = O.tkl_params_from_state({k: v.cpu() for k, v in m.state_dict().items()})
        ref, ref_win = O.tkl_forward_bypass(s["q"].numpy(), s["d"].numpy(), s["qm"].numpy(), s["dm"].numpy(), params, s["sat"],
                                            dtype=np.float64, return_windows=True)
        util.tkl_check_documents(_np(score), _np(win), _np(peaks), ref, ref_win, _np(m.chunk_scoring).reshape(-1), label="poisoned tkl")
        assert not win[1].any() and float(score[1]) == 0.0, "the empty document"
    st = {"run": run, "check": check}
    if chain:
        st["ints"] = lambda out: [("peaks", out[2], 0, max(out[1].shape[1], 3))]
        st["next"] = lambda out: [_tkl_bwd_stage(s, out[1])]
    return st


def _tkl_bwd_stage(s, win):
    from matchmaker_amd import ops
    from tests.tkl_window_reference import selected_window_scores
    m = s["m"]

    def run():
        return ops.tkl_bwd(s["q_ctx"], s["chunks"], s["cmask"], s["slot"], s["qmd"], m.pack_params(), win, s["go"], s["B"], s["C"], 11, s["sat"])

    def check(out):          # tests/test_tkl_gpu.py::test_native_backward_equals_the_differentiable_torch_restatement
        gq, gc, gp = out
        for p in m.parameters():
            p.grad = None
        q_t = s["q_ctx"].detach().clone().requires_grad_(True)
        c_t = s["chunks"].detach().clone().requires_grad_(True)
        sc = selected_window_scores(m, q_t, c_t, s["cmask"], s["slot"], s["qmd"], win.detach().clone(), s["C"])
        (sc * s["go"]).sum().backward()
        pairs = [(gq, q_t.grad, "grad_q"), (gc, c_t.grad, "grad_chunks")]
        scoring, sizes = m._pack_layout()
        for t, n in zip(scoring, sizes):
            if n is not None and t.grad is not None:
                pairs.append((gp[n[0]:n[0] + n[1]], t.grad.reshape(-1)[:n[1]], f"grad_params[{n[0]}:{n[0] + n[1]}]"))
        assert len(pairs) > 3
        for got, want, name in pairs:
            scale = max(1.0, float(want.abs().max()))
            torch.testing.assert_close(got, want, rtol=2e-3, atol=3e-4 * scale, msg=lambda m_, n=name: f"{n}: {m_}")
        assert not gq[1].any(), "the empty document sends no gradient to its query"
    return {"name": "tkl_bwd", "run": run, "check": check}


def _tkl_case(sat, D, what):
    def build(dev):
        s = _tkl_setup(dev, sat, D)
        if what == "bwd":
            from matchmaker_amd import ops
            _, win = ops.tkl_score(s["q_ctx"], s["chunks"], s["cmask"], s["slot"], s["qmd"], s["m"].pack_params(), s["B"], s["C"], 11,
                                   sat, return_windows=True)
            return _tkl_bwd_stage(s, win)
        return _tkl_fwd_stage(s, what == "chain")
    return build


case("tkl_score-embedding-D300", "tkl_score")(_tkl_case("embedding", 300, "fwd"))
case("tkl_score-log-D120", "tkl_score")(_tkl_case("log", 120, "fwd"))
case("tkl_bwd-embedding-D300", "tkl_bwd")(_tkl_case("embedding", 300, "bwd"))
case("chain-tkl_score->tkl_bwd-embedding-D300", "tkl_score", "tkl_bwd")(_tkl_case("embedding", 300, "chain"))
case("chain-tkl_score->tkl_bwd-log-D120", "tkl_score", "tkl_bwd")(_tkl_case("log", 120, "chain"))


# ======================================================================================================= flat top-k, merge
# (nq, N, E, k, store): a store smaller than k and one a little larger, nq = 1 and 37, one past the sampling switch (N > 4096)
TOPK = [(1, 7, 128, 10, "ternary"), (37, 7, 128, 10, "quarter"), (1, 13, 256, 10, "quarter"), (37, 13, 128, 10, "ternary"),
        (37, 5000, 128, 10, "ternary")]


def _dot_topk_case(nq, N, E, k, kind):
    def build(dev):
        from matchmaker_amd import ops
        from tests import dot_topk_reference as R
        q, c = R.inputs(kind, nq, N, E, seed=nq + N)
        ref = R.dot_topk_exact(q, c, k)
        a = (_t(q, dev, torch.float16), _t(c, dev, torch.float16))
        # tests/test_dot_topk_exact_gpu.py::test_instantiations_bit_equal_with_ties
        return {"run": lambda: ops.dot_topk(*a, k), "check": lambda out: _equal(out, ref, "dot_topk")}
    return build


def _dot_topk_fp8_case(nq, N, E, k, kind):
    def build(dev):
        from matchmaker_amd import ops
        from tests import fp8_token_search_reference as R
        q, codes, scales = R.scaled_store(nq, N, E, seed=nq + N)
        ref = R.dot_topk_fp8_exact(q, codes, scales, k)
        a = (_t(q, dev, torch.bfloat16), _t(codes, dev), _t(scales, dev))
        # tests/test_fp8_token_search_gpu.py::test_scaled_store_bit_equal_with_ties
        return {"run": lambda: ops.dot_topk_fp8(*a, k), "check": lambda out: _equal(out, ref, "dot_topk_fp8")}
    return build


for _c in TOPK:
    case("dot_topk-nq{}-N{}-E{}-k{}".format(*_c), "dot_topk")(_dot_topk_case(*_c))
    case("dot_topk_fp8-nq{}-N{}-E{}-k{}".format(*_c), "dot_topk_fp8")(_dot_topk_fp8_case(*_c))


def _merge_case(n_in, k):
    def build(dev):
        from matchmaker_amd import ops
        from tests import dot_topk_reference as R
        s, ids = R.merge_inputs(n_in)          # a row of padding only; ids above 2^40
        ref = R.topk_merge_exact(s, ids, k)
        a = (_t(s, dev), _t(ids, dev))
        # tests/test_dot_topk_exact_gpu.py::test_topk_merge_bit_equal_with_ties_padding_and_wide_ids
        return {"run": lambda: ops.topk_merge(*a, k), "check": lambda out: _equal(out, ref, "topk_merge")}
    return build


case("topk_merge-n7-k10", "topk_merge")(_merge_case(7, 10))
case("topk_merge-n1000-k13", "topk_merge")(_merge_case(1000, 13))


# ======================================================================================================= IVF scans
def _ivf_problem(which):
    """The exact store over tests/test_ivf_gpu.py's lists (empty lists, one and two blocks, partial last blocks): (1) one
    query, (37) 37 queries, (short) unions of 16 / 0 / 17 / 31 / 0 rows under k = 100 — fewer than k survivors, an empty list
    alone, a query that probes nothing."""
    from tests import fp8_token_search_reference as R
    from tests import ivf_fp8_reference as I8
    if which == "short":
        q, codes, scales = R.scaled_store(5, I8.N_ROWS, 128, 11)
        return q, codes, scales, I8.list_begin(), I8.short_union_probes(), 100
    nq, k = (1, 1) if which == "1" else (37, 10)
    q, codes, scales, lb, probes = I8.exact_problem(128, nq, I8.EXACT_NPROBE, I8.exact_seed(128, nq, k))
    return q, codes, scales, lb, probes, k


def _ivf_case(which, fp8):
    def build(dev):
        from matchmaker_amd import ops
        from tests import ivf_fp8_reference as I8
        q, codes, scales, lb, probes, k = _ivf_problem(which)
        ref_s, ref_r = I8.ivf_scan_fp8(q, codes, scales, lb, probes, k)
        qd, cd, sd, lbd, pd = _t(q, dev, torch.float16), _t(codes, dev), _t(scales, dev), _t(lb, dev), _t(probes, dev)
        if fp8:
            run = lambda: ops.ivf_scan_fp8(qd, cd, sd, lbd, pd, k)      # noqa: E731
        else:                # the dequantised rows are exact in fp16 (|value| <= 64): the same scores, tests/test_ivf_fp8_gpu.py
            v = ops.fp8_dequantize_rows(cd, sd, torch.float16)
            run = lambda: ops.ivf_scan(qd, v, lbd, pd, k)               # noqa: E731
        # tests/test_ivf_fp8_gpu.py::test_scan_equals_the_restatement_bit_for_bit_on_the_exact_store, ::test_scan_equals_the_16_bit_scan_of_the_dequantised_rows
        return {"run": run, "check": lambda out: _equal(out, (ref_s, ref_r), "ivf_scan")}
    return build


for _w in ("1", "37", "short"):
    case(f"ivf_scan-{_w}", "ivf_scan")(_ivf_case(_w, False))
    case(f"ivf_scan_fp8-{_w}", "ivf_scan_fp8")(_ivf_case(_w, True))


# ======================================================================================================= quantized index
def _ah_scan_case(nq, k, short):
    def build(dev):
        from matchmaker_amd import ops
        from tests import scann_reference as SR
        from tests.test_scann_gpu import _check_union, _problem, _tol
        E = 128
        q, codes, cb, lb, probes, ps, _ = _problem(torch.float16, E, nq, 4 if short else 6, seed=E + nq + k)
        if short:            # tests/test_scann_gpu.py::test_ah_scan_k_larger_than_the_union_and_empty_rows
            probes[:] = -1
            probes[0, :2] = [1, 2]
            probes[1, 0] = 0
            probes[2, :3] = [6, 0, 4]
            probes[3, 2] = 12
        a = (q.to(dev), codes.to(dev), cb.to(dev), _t(lb, dev), _t(probes, dev), ps.to(dev))
        dec = SR.decode(codes.numpy(), cb.float().numpy())

        def check(out):      # tests/test_scann_gpu.py::test_ah_scan_is_the_exact_topk_of_the_probed_union
            _check_union(q.float().numpy(), dec, lb, probes, ps.numpy(), k, _np(out[0]), _np(out[1]), tol=_tol(E))
        return {"run": lambda: ops.ah_scan(*a, k), "check": check}
    return build


case("ah_scan-nq1-k1", "ah_scan")(_ah_scan_case(1, 1, False))
case("ah_scan-nq37-k10", "ah_scan")(_ah_scan_case(37, 10, False))
case("ah_scan-short-unions-k100", "ah_scan")(_ah_scan_case(5, 100, True))


@case("ah_encode-exact-n67-E128", "ah_encode")
def _ah_encode(dev):
    from matchmaker_amd import ops
    from tests import scann_reference as SR
    from tests.test_scann_gpu import eta_of, plant_exact_rows
    E = 128
    x, lists, cent, cb = SR.exact_store(67, E, 7, seed=5)
    x, lists, cent = plant_exact_rows(x, lists, cent, cb)
    ref = SR.encode(x, lists, cent, cb, eta_of(E), 2)
    a = (_t(x, dev, torch.float16), _t(lists, dev), _t(cent, dev, torch.float16), _t(cb, dev, torch.float16))
    # tests/test_scann_gpu.py::test_ah_encode_is_bit_equal_to_the_restatement_on_an_exact_store
    return {"run": lambda: ops.ah_encode(*a, eta_of(E), 2), "check": lambda out: np.testing.assert_array_equal(_np(out), ref)}


def _gather_dot_case(nq, R_):
    def build(dev):
        from matchmaker_amd import ops
        from tests import scann_reference as SR
        from tests.test_scann_gpu import _tol
        E, n = 128, 300
        g = torch.Generator().manual_seed(E + nq + R_)
        v = torch.randn(n, E, generator=g).half()
        q = torch.randn(nq, E, generator=g).half()
        rows = torch.randint(0, n, (nq, R_), generator=g)
        rows[torch.rand(nq, R_, generator=g) < 0.1] = -1
        rows[0, 0] = -1
        rows[-1, -1] = n - 1
        ref = SR.gather_dot(q.float().numpy(), v.float().numpy(), rows.numpy())
        hole = rows.numpy() < 0
        a = (q.to(dev), v.to(dev), rows.to(dev))

        def check(out):      # tests/test_scann_gpu.py::test_gather_dot_is_the_exact_inner_product
            out = _np(out)
            assert np.isneginf(out[hole]).all() and np.isfinite(out[~hole]).all()
            np.testing.assert_allclose(out[~hole], ref[~hole], atol=_tol(E), rtol=1e-3)
        return {"run": lambda: ops.gather_dot(*a), "check": check}
    return build


case("gather_dot-nq1-R3", "gather_dot")(_gather_dot_case(1, 3))
case("gather_dot-nq37-R33", "gather_dot")(_gather_dot_case(37, 33))


# ======================================================================================================= graph index
def _graph_case(nq, k, ef, dead_ends):
    def build(dev):
        from matchmaker_amd import ops
        from tests import graph_reference as GR
        from tests.test_graph_gpu import _assert_equal, _entries, _queries, _store
        x, g = _store(1500, 128, 8)
        q = _queries(nq, 128, seed=1000 + nq)
        e = _entries(nq, 1500, 8, seed=1500 + nq)
        width = 2
        if dead_ends:        # tests/test_graph_gpu.py::test_search_edge_cases_equal_the_restatement: k rows are never reached
            g = np.full_like(g, -1)
            e[0, 1] = e[0, 0]
            e[-1, ::2] = -1
            if nq > 2:
                e[2, :] = -1
        ref = GR.search(x, g, q, e, ef, width, GR.default_max_iters(ef, width), k)
        a = (_t(q, dev, torch.float16), _t(x, dev, torch.float16), _t(g, dev), _t(e, dev))

        def check(out):      # tests/test_graph_gpu.py::test_search_is_bit_equal_to_the_restatement_on_exact_stores
            _assert_equal(tuple(_np(t) for t in out), ref, "graph_search")
        return {"run": lambda: ops.graph_search(*a, ef, k, width, return_stats=True), "check": check}
    return build


case("graph_search-nq1-k10", "graph_search")(_graph_case(1, 10, 32, False))
case("graph_search-nq37-k10", "graph_search")(_graph_case(37, 10, 32, False))
case("graph_search-nq37-k32-dead-ends", "graph_search")(_graph_case(37, 32, 32, True))


# ======================================================================================================= k-means
def _kmeans_assign_case(n, nlist):
    def build(dev):
        from matchmaker_amd import ops
        from tests.test_kmeans_gpu import _exact_problem
        x, c, a_ref, s_ref = _exact_problem(n, 128, nlist)
        a = (_t(x, dev, torch.float16), _t(c, dev, torch.float16))

        def check(out):      # tests/test_kmeans_gpu.py::test_assignment_shapes_on_the_exact_store
            assert (_np(out[0]) == a_ref).all() and (_np(out[1]).astype(np.float64) == s_ref).all()
        return {"run": lambda: ops.kmeans_assign(*a), "check": check}
    return build


def _kmeans_sum_case(n):
    def build(dev):
        from matchmaker_amd import ops
        from tests import kmeans_reference as KR
        x = KR.exact_store(n, 128, seed=3)
        if n == 1:
            order, lb = np.zeros(1, np.int64), np.array([0, 0, 1, 1], np.int64)
        else:                # empty lists at the start, in the middle and at the end; rows outside [0, n) are skipped
            order = np.random.default_rng(4).permutation(n).astype(np.int64)
            order[[0, 17]] = [-1, n + 5]
            lb = np.array([0, 0, 120, 120, 121, n, n], np.int64)
        ref = KR.segment_sum(x, order, lb)
        a = (_t(x, dev, torch.float16), _t(order, dev), _t(lb, dev))

        def check(out):      # tests/test_kmeans_gpu.py::_check_exact_sums
            assert (_np(out).astype(np.float64) == ref).all()
        return {"run": lambda: ops.kmeans_segment_sum(*a), "check": check}
    return build


case("kmeans_assign-n1", "kmeans_assign")(_kmeans_assign_case(1, 37))
case("kmeans_assign-n300", "kmeans_assign")(_kmeans_assign_case(300, 130))
case("kmeans_segment_sum-n1", "kmeans_segment_sum")(_kmeans_sum_case(1))
case("kmeans_segment_sum-n300-empty-clusters", "kmeans_segment_sum")(_kmeans_sum_case(300))


# ======================================================================================================= ColBERT retrieval
def _candidates_setup(dev):
    from tests import colbert_search_reference as R
    from tests.test_colbert_search_gpu import _layout
    rng = np.random.default_rng(4)
    begin, end, T = _layout(rng, 40)             # gaps, zero-length documents, a permuted document order
    hits = rng.integers(-2, T + 3, (4, 90))
    hits[rng.random(hits.shape) < 0.1] = -1
    hits[2] = -1                                 # a query without any hit: count 0, every slot a pad
    bs, es, dof = R.sorted_view(begin, end)
    cap = min(hits.shape[1], len(bs))
    want = R.padded_candidates(R.candidates_ref(hits, begin, end), begin, end, cap)
    return hits, begin, end, T, (_t(hits, dev), _t(bs, dev), _t(es, dev), _t(dof, dev)), want


def _candidates_stage(dev, chain):
    from matchmaker_amd import ops
    hits, begin, end, T, a, want = _candidates_setup(dev)

    def check(out):          # tests/test_colbert_search_gpu.py::_check_kernel
        for name, g, w in zip(("cand_doc", "cand_begin", "cand_end", "count"), out, want):
            assert _np(g).dtype == w.dtype and np.array_equal(_np(g), w), name
    st = {"run": lambda: ops.colbert_candidates(*a, T), "check": check}
    if chain:
        rng = np.random.default_rng(9)
        E, Q = 128, 13
        tok = torch.from_numpy(rng.standard_normal((T, E)).astype(np.float32)).to(torch.bfloat16)
        q = torch.from_numpy(rng.standard_normal((hits.shape[0], Q, E)).astype(np.float32) / np.sqrt(E)).to(torch.bfloat16)
        q_len = torch.tensor([Q, 7, 1, Q], dtype=torch.int32)
        qd, tokd, qld = q.to(dev), tok.to(dev), q_len.to(dev)

        def consumer(out):
            _, cb, ce, _ = out
            cap = cb.shape[1]
            ref = _ragged_ref(q, q_len, tok, _np(cb).reshape(-1), _np(ce).reshape(-1), cap)

            def check2(s):   # tests/test_maxsim_ragged_bwd_gpu.py::test_ragged_matches_per_document_aggregation
                assert (np.abs(_np(s) - ref) <= util.TOL_BF16 + 1e-4 * np.abs(ref)).all()
            return [{"name": "maxsim_ragged", "check": check2,
                     "run": lambda: ops.maxsim_ragged(qd, tokd, cb.reshape(-1), ce.reshape(-1), qld, pairs_per_query=cap)}]
        st["ints"] = lambda out: [("cand_doc", out[0], -1, len(begin)), ("cand_begin", out[1], 0, T + 1), ("cand_end", out[2], 0, T + 1),
                                  ("end - begin", out[2] - out[1], 0, T + 1), ("count", out[3], 0, out[0].shape[1] + 1)]
        st["next"] = consumer
    return st


case("colbert_candidates-nq4-H90", "colbert_candidates")(lambda dev: _candidates_stage(dev, False))
case("chain-colbert_candidates->maxsim_ragged", "colbert_candidates", "maxsim_ragged")(lambda dev: _candidates_stage(dev, True))


def _untouched(t, poison_byte, label):
    assert bool((t.contiguous().view(torch.uint8) == poison_byte).all()), f"store_append wrote {label}"


def _store_append_case(dtype, fp8, keep_zero):
    """The store's buffers come from the poisoned arena too (ops.torch is the proxy while the case runs), so their guards take
    part in the overrun check, and the rows outside [old fill, new fill) — which the operator must leave alone — are checked to
    hold the poison still.  The bit comparison covers what it owns: the appended rows, the ranges, fill and status."""
    def build(dev):
        from matchmaker_amd import ops
        from tests import store_writer_reference as W
        n_docs, D, E, cap, fill0 = 9, 5, 48, 60, 3
        x = W.pattern_batch(n_docs, D, E, dtype, seed=7)          # fully live, all-zero, one-live-row, -0.0, subnormal documents
        xd = x.to(dev)

        def buffers(empty, device):
            rows = empty((cap, E), dtype=dtype, device=device)
            codes = empty((cap, E), dtype=torch.uint8, device=device) if fp8 else None
            scales = empty((cap,), dtype=torch.float32, device=device) if fp8 else None
            fill = empty((1,), dtype=torch.int64, device=device)
            status = empty((1,), dtype=torch.int32, device=device)
            begin = empty((n_docs,), dtype=torch.int64, device=device)
            end = empty((n_docs,), dtype=torch.int64, device=device)
            return rows, codes, scales, fill, begin, end, status

        def run():
            rows, codes, scales, fill, begin, end, status = buffers(ops.torch.empty, dev)
            poison_byte = int(rows.view(torch.uint8).flatten()[0])
            fill.fill_(fill0)
            status.zero_()
            ops.store_append(xd, rows, codes, scales, cap, fill, begin, end, status, keep_zero_rows=keep_zero)
            T = int(fill[0])
            assert fill0 <= T <= cap
            for name, t in (("rows", rows), ("codes", codes), ("scales", scales)):
                if t is not None:
                    _untouched(t[:fill0], poison_byte, f"{name} below the old fill")
                    _untouched(t[T:], poison_byte, f"{name} past the new fill")
            return {"rows": rows[fill0:T], "codes": None if codes is None else codes[fill0:T],
                    "scales": None if scales is None else scales[fill0:T], "fill": fill, "begin": begin, "end": end, "status": status}

        def check(got):      # tests/test_store_writer_gpu.py::test_rows_ranges_and_fill_equal_the_restatement, ::test_fp8_output_equals_...
            cpu = buffers(lambda size, dtype, device: torch.zeros(size, dtype=dtype), None)
            cpu[3].fill_(fill0)
            W.append_standin(x, cpu[0], cpu[1], cpu[2], cap, cpu[3], cpu[4], cpu[5], cpu[6], keep_zero_rows=keep_zero)
            want = dict(zip(["rows", "codes", "scales", "fill", "begin", "end", "status"], cpu))
            T = int(want["fill"][0])
            assert fill0 < T <= cap and int(got["fill"][0]) == T and int(got["status"][0]) == 0
            assert torch.equal(W.bits(got["rows"].cpu()), W.bits(want["rows"][fill0:T])), "rows"
            if fp8:
                from tests import fp8_store_reference as R8
                assert torch.equal(R8.fold_zero(got["codes"].cpu()), R8.fold_zero(want["codes"][fill0:T])), "codes"
                assert torch.equal(got["scales"].cpu(), want["scales"][fill0:T]), "scales"
            assert torch.equal(got["begin"].cpu(), want["begin"]) and torch.equal(got["end"].cpu(), want["end"]), "document ranges"
        return {"run": lambda: [v for v in run().values() if v is not None],
                "check": lambda out: check(dict(zip(["rows"] + (["codes", "scales"] if fp8 else []) + ["fill", "begin", "end", "status"], out)))}
    return build


case("store_append-bf16-rows", "store_append")(_store_append_case(torch.bfloat16, False, False))
case("store_append-f32-rows+fp8-keep-zero", "store_append")(_store_append_case(torch.float32, True, True))
case("store_append-f16-rows+fp8", "store_append")(_store_append_case(torch.float16, True, False))


@case("store_append-all-zero-batch", "store_append")
def _store_append_zeros(dev):
    from matchmaker_amd import ops
    z = torch.zeros(5, 7, 48, dtype=torch.float16, device=dev)

    def run():
        e = ops.torch.empty
        rows, fill, status = e((20, 48), dtype=torch.float16, device=dev), e((1,), dtype=torch.int64, device=dev), e((1,), dtype=torch.int32, device=dev)
        begin, end = e((5,), dtype=torch.int64, device=dev), e((5,), dtype=torch.int64, device=dev)
        poison_byte = int(rows.view(torch.uint8).flatten()[0])
        fill.fill_(17)
        status.zero_()
        ops.store_append(z, rows, None, None, 20, fill, begin, end, status)
        _untouched(rows, poison_byte, "rows although every row of the batch is zero")
        return fill, begin, end, status

    def check(out):          # tests/test_store_writer_gpu.py::test_a_whole_batch_of_zeros_and_keep_zero_rows
        assert int(out[0]) == 17 and int(out[3]) == 0 and bool((out[1] == 17).all()) and bool((out[2] == 17).all())
    return {"run": run, "check": check}


# ======================================================================================================= PACRR family
def _pacrr_inputs(dev, nq, ppq, B, Q, D, E, C, N, k, lens=None):
    from tests.test_pacrr_gpu import _params
    g = torch.Generator().manual_seed(Q * 7 + D + E + C + N + k)
    q = torch.randn(nq, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    if lens is not None:
        d = d * (torch.arange(D)[None, :, None] < torch.tensor(lens)[:, None, None])
    ws, bs = _params(g, C, N, dev)
    return q.to(dev), d.to(dev), ws, bs, g


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _pacrr_stage(dev, shape, lens, chain):
    """tests/test_pacrr_gpu.py::test_random_sweep_forward_and_backward_against_fp64 and
    ::test_zero_padded_documents_backward_and_the_tie_policy"""
    from matchmaker_amd import ops
    from tests import pacrr_reference as P
    from tests.test_pacrr_gpu import TOL_PQR
    nq, ppq, B, Q, D, E, C, N, k = shape
    q, d, ws, bs, g = _pacrr_inputs(dev, *shape, lens=lens)
    q64, d64 = q.double().requires_grad_(True), d.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws]
    b64 = [b.double().requires_grad_(True) for b in bs]
    ref, cols, chans = P.per_query_results(q64, d64, w64, b64, k, ppq, return_positions=True)
    gout = torch.randn(ref.shape, generator=g).to(dev)

    def check(out):
        o, idx = out
        assert tuple(o.shape) == (B, Q, k * N) and float((o.double() - ref.detach()).abs().max()) < TOL_PQR
        if lens is None:
            assert float(((idx.long() & 0xffff) == cols).double().mean()) > 0.999
            assert float(((idx.long() >> 16) == chans).double().mean()) > 0.999
    st = {"run": lambda: ops.pacrr_kmax(q, d, ws, bs, k, ppq, save=True), "check": check}

    def consumer(out):
        idx = out[1]

        def check2(res):
            gq, gd, gw, gb = res
            if q64.grad is None:
                (ref * gout.double()).sum().backward()
            assert all(torch.isfinite(t).all() for t in [gq, gd] + gw + gb)
            assert _rel(gq, q64.grad) < 1e-4
            if lens is None:
                assert _rel(gd, d64.grad) < 1e-4
            else:            # padded rows tie exactly: compared as their sum (the tie policy of the zero-padded test)
                pad = (torch.arange(D)[None, :] >= torch.tensor(lens)[:, None]).to(dev)
                assert _rel(gd[~pad], d64.grad[~pad]) < 1e-4
                for b in range(B):
                    if pad[b].any():
                        assert _rel(gd[b][pad[b]].sum(0), d64.grad[b][pad[b]].sum(0)) < 1e-4
            for a, b in zip(gw + gb, w64 + b64):
                assert _rel(a, b.grad) < 1e-4
        return [{"name": "pacrr_kmax_bwd", "run": lambda: ops.pacrr_kmax_bwd(q, d, ws, idx, gout, k, ppq), "check": check2}]
    if chain:
        st["ints"] = lambda out: [("idx columns", out[1] & 0xffff, 0, D), ("idx channels", out[1] >> 16, 0, max(C, 1))]
        st["next"] = consumer
    return st


# the smallest rows of tests/test_pacrr_gpu.py's SWEEP, and its zero-padded documents (lengths 200 / 90 / 40 / 17 under k = 16)
PACRR = [("Q1-D33-N2", (2, 1, 2, 1, 33, 64, 16, 2, 5), None), ("D16=k-N1", (2, 1, 2, 30, 16, 64, 16, 1, 16), None),
         ("D1-k1", (2, 1, 2, 64, 1, 768, 64, 2, 1), None), ("zero-padded", (4, 1, 4, 30, 200, 300, 32, 3, 16), [200, 90, 40, 17])]
for _n, _s, _l in PACRR:
    case("pacrr_kmax-" + _n, "pacrr_kmax")(lambda dev, s=_s, l=_l: _pacrr_stage(dev, s, l, False))
    case("chain-pacrr_kmax->pacrr_kmax_bwd-" + _n, "pacrr_kmax", "pacrr_kmax_bwd")(lambda dev, s=_s, l=_l: _pacrr_stage(dev, s, l, True))


def _co_pacrr_stage(dev, shape, lens, chain):
    """tests/test_co_pacrr_gpu.py::test_random_sweep_forward_and_backward_against_fp64"""
    from matchmaker_amd import ops
    from tests import co_pacrr_reference as CP
    from tests.test_co_pacrr_gpu import TOL_PQR, _fp64, _value_mask
    nq, ppq, B, Q, U, D, E, C, N, k = shape
    q, d, ws, bs, g = _pacrr_inputs(dev, nq, ppq, B, Q, D, E, C, N, k + U, lens=lens)
    views = ops.co_pacrr_views(U)
    q64, d64, w64, b64, ref, mats = _fp64(q, d, ws, bs, k, U, ppq)
    vm = _value_mask(k, N)
    gout = torch.randn(ref.shape, generator=g).to(dev)
    state = {}

    def check(out):
        o, idx = out
        assert tuple(o.shape) == (B, Q, 8 * k * N) and tuple(idx.shape) == (B, Q, N, 4 * k)
        assert float((o[..., vm].double().cpu() - ref.detach()[..., vm].cpu()).abs().max()) < TOL_PQR
        n_ex, tied = CP.compare_context_slots(o, ref, mats, k, U, atol=TOL_PQR, return_pairs=True)
        if lens is None:
            assert n_ex <= 0.001 * o.numel() / 2
        state["tied"] = tied
    st = {"run": lambda: ops.co_pacrr_kmax(q, d, ws, bs, k, views, ppq, save=True), "check": check}

    def consumer(out):
        idx = out[1]
        go = gout.clone()
        go[state["tied"].to(dev)] = 0.0          # a near-tie across the k-th place may route its gradient to another column

        def check2(res):
            gq, gd, gw, gb = res
            if q64.grad is None:
                (ref * go.double()).sum().backward()
            assert all(torch.isfinite(t).all() for t in [gq, gd] + gw + gb)
            assert _rel(gq, q64.grad) < 1e-4 and _rel(gd, d64.grad) < 1e-4
            for a, b in zip(gw + gb, w64 + b64):
                assert _rel(a, b.grad) < 1e-4
        return [{"name": "co_pacrr_kmax_bwd", "run": lambda: ops.co_pacrr_kmax_bwd(q, d, ws, idx, go, k, views, ppq), "check": check2}]
    if chain:
        st["ints"] = lambda out: [("idx columns", out[1] & 0xffff, 0, D), ("idx channels", out[1] >> 16, 0, max(C, 1))]
        st["next"] = consumer
    return st


# the smallest rows of tests/test_co_pacrr_gpu.py's SWEEP (Q = 1 / k = 1; D below the first view; an odd U)
CO_PACRR = [("Q1-k1-D9", (2, 1, 2, 1, 4, 9, 64, 8, 2, 1)), ("D37-below-v0", (2, 1, 2, 30, 200, 37, 64, 16, 3, 5)),
            ("odd-U30-D45", (2, 1, 2, 17, 30, 45, 64, 16, 4, 7))]
for _n, _s in CO_PACRR:
    case("co_pacrr_kmax-" + _n, "co_pacrr_kmax")(lambda dev, s=_s: _co_pacrr_stage(dev, s, None, False))
    case("chain-co_pacrr_kmax->co_pacrr_kmax_bwd-" + _n, "co_pacrr_kmax", "co_pacrr_kmax_bwd")(lambda dev, s=_s: _co_pacrr_stage(dev, s, None, True))


@case("co_pacrr_kmax-zero-padded", "co_pacrr_kmax")
def _co_pacrr_zero_padded(dev):
    """Zero-padded documents (the zero columns tie exactly): the value slots against fp64, the context slots under the
    reference's own tie rule (compare_context_slots); the backward of tied columns is PACRR's policy and is run there."""
    return _co_pacrr_stage(dev, (3, 1, 3, 30, 200, 120, 64, 16, 3, 5), [120, 60, 33], False)


# ======================================================================================================= DRMM
def _drmm_case(nq, ppq, B, Q, D, E, bins, lens, score):
    def build(dev):
        from matchmaker_amd import ops
        from tests import drmm_reference as DR
        from tests.test_drmm_cpu import CAP
        from tests.test_drmm_gpu import _head64
        g = torch.Generator().manual_seed(Q * 7 + D + E + bins + B)
        q = torch.randn(nq, Q, E, generator=g)
        d = torch.randn(B, D, E, generator=g)
        d[:, ::13] = 0
        d_len = None
        if lens:             # zero-padded documents, one of them empty
            d_len = torch.randint(1, D + 1, (B,), generator=g).to(torch.int32)
            d_len[-1] = 0
            d = d * (torch.arange(D)[None, :, None] < d_len[:, None, None]).float()
        tol = DR.measured_tol(q, d, ppq)
        bd = DR.bounds(q, d, bins, tol, ppq)
        assert bd["share"] <= CAP
        qd, dd = q.to(dev), d.to(dev)
        dl = d_len.to(dev) if lens else None
        if not score:        # tests/test_drmm_gpu.py::test_random_sweep_against_the_decided_bounds
            return {"run": lambda: ops.drmm_hist(qd, dd, bins, ppq, d_len=dl), "check": lambda out: DR.check_hist(out, bd, tol, "poisoned")}
        W1, b1 = torch.randn(bins, bins, generator=g).to(dev), torch.randn(bins, generator=g).to(dev)
        w2, b2 = torch.randn(1, bins, generator=g).to(dev), torch.randn(1, generator=g).to(dev)
        gate = torch.softmax(torch.randn(nq, Q, generator=g), dim=-1).to(dev)

        def check(out):      # the fused head: 1e-5 against the fp64 head on the kernel's own histogram (same test)
            s, hist = out
            DR.check_hist(hist, bd, tol, "poisoned")
            assert float((s.double().cpu() - _head64(hist, DR.expand_queries(gate, B, ppq), W1, b1, w2, b2)).abs().max()) <= 1e-5
        return {"run": lambda: ops.drmm_score(qd, dd, gate, W1, b1, w2, b2, ppq, d_len=dl, return_hist=True), "check": check}
    return build


# the smallest rows of tests/test_drmm_gpu.py's SWEEP (Q = 1, D = 1; Q = 17 with lengths; the partial last group)
DRMM = [("Q1-D1", (2, 1, 2, 1, 1, 64, 10, False)), ("Q17-D77-zero-padded", (2, 1, 2, 17, 77, 200, 16, True)),
        ("ppq3-Q20-D70-E36-zero-padded", (2, 3, 5, 20, 70, 36, 7, True))]
for _n, _s in DRMM:
    case("drmm_hist-" + _n, "drmm_hist")(_drmm_case(*_s, score=False))
    case("drmm_score-" + _n, "drmm_score")(_drmm_case(*_s, score=True))


# ======================================================================================================= MatchPyramid
def _matchpyramid_case(nq, ppq, B, Q, D, E, channels, kernels, pools):
    def build(dev):
        from matchmaker_amd import ops
        from tests import matchpyramid_reference as MR
        from tests.test_matchpyramid_gpu import _check
        g = torch.Generator().manual_seed(Q * 7 + D + E + B)
        q = torch.randn(nq, Q, E, generator=g)
        d = torch.randn(B, D, E, generator=g)
        d[:, ::13] = 0                            # zero rows (row 0 of every document among them)
        p = MR.random_params(channels, kernels, pools, seed=Q + D, scale=2.0)
        w, b = MR.conv_lists(p)
        a = (q.to(dev), d.to(dev), [t.to(dev) for t in w], [t.to(dev) for t in b], p["pools"], ppq)
        # tests/test_matchpyramid_gpu.py::test_random_sweep_against_fp64
        return {"run": lambda: ops.matchpyramid_features(*a), "check": lambda out: _check(out, q, d, p, "poisoned", ppq)}
    return build


case("matchpyramid_features-Q1-D1", "matchpyramid_features")(_matchpyramid_case(2, 1, 2, 1, 1, 16, [3, 2], [[1, 1], [3, 3]], [[2, 2], [1, 1]]))
case("matchpyramid_features-Q9-D23-5x5", "matchpyramid_features")(_matchpyramid_case(2, 1, 2, 9, 23, 16, [6, 7], [[5, 5], [5, 5]], [[5, 11], [3, 4]]))
case("matchpyramid_features-ppq3-Q8-D20", "matchpyramid_features")(_matchpyramid_case(2, 3, 5, 8, 20, 30, [4, 4], [[3, 3], [3, 3]], [[4, 8], [2, 3]]))


def _matchpyramid_chain(name):
    """tests/test_matchpyramid_bwd_gpu.py: the features against fp64 (MR.measured_tol), the saved arg-max inside its conv plane,
    the gradients against the given-arg-max form fed the kernel's own indices (BR.tol)."""
    def build(dev):
        from matchmaker_amd import ops
        from tests import matchpyramid_bwd_reference as BR
        from tests import matchpyramid_reference as MR
        from tests.test_matchpyramid_bwd_gpu import _compare, _on, per_layer
        q, d, go, w, b, pools = _on(dev, name)

        def check(out):
            f, (pooled, argmax) = out
            f64 = BR.oracle_a(name, torch.float64)["features"]
            assert float((f.double().cpu() - f64).abs().max()) <= MR.measured_tol(BR.oracle_a(name, torch.float32)["features"], f64)
            last = per_layer(name, pooled.cpu())[-1]
            assert torch.equal(last.reshape(last.shape[0], -1), f.cpu())

        def limits(out):     # per layer the arg-max indexes its channel's Ho x Wo conv plane
            arg = per_layer(name, out[1][1].cpu())
            return [(f"argmax of layer {l}", a_, 0, geo[6] * geo[7]) for l, (a_, geo) in enumerate(zip(arg, BR.geometry(name)))]

        def consumer(out):
            saved = out[1]

            def check2(res):
                gq, gd, gw, gb = res
                got = {"gq": gq.cpu(), "gd": gd.cpu(), "gw": [t.cpu() for t in gw], "gb": [t.cpu() for t in gb]}
                arg = [a_.long() for a_ in per_layer(name, saved[1].cpu())]
                _compare(name, got, BR.oracle_b(name, torch.float32, arg), BR.oracle_b(name, torch.float64, arg))
            return [{"name": "matchpyramid_bwd", "run": lambda: ops.matchpyramid_bwd(q, d, w, b, pools, saved, go), "check": check2}]
        return {"run": lambda: ops.matchpyramid_features_save(q, d, w, b, pools), "check": check, "ints": limits, "next": consumer}
    return build


for _n in ("tiny", "zero", "up", "rect"):
    case(f"chain-matchpyramid_features_save->matchpyramid_bwd-{_n}", "matchpyramid_features_save", "matchpyramid_bwd")(_matchpyramid_chain(_n))


# ======================================================================================================= ranking and metrics
def _rank_setup(dev, dtype):
    from tests import rank_metrics_reference as RR
    lengths = [0, 1, 64, 65, 0]
    sb = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=sb[1:])
    n, nq = int(sb[-1]), len(lengths)
    rng = np.random.default_rng(12)
    scores = (rng.integers(0, 9, n).astype(np.float32) - 4) / 2       # many ties; exact in every dtype
    scores[5], scores[70] = np.nan, -0.0
    grade = rng.choice(np.array([RR.NOT_JUDGED, 0, 0, 1, 2, 3], np.int64), n).astype(np.int32)
    cand_pos = np.concatenate([rng.permutation(l) + 1 for l in lengths]).astype(np.int32)
    binp, rcut, ncut, map_cut = 1, [1, 10, 100], [3, 10], 1000
    bnr = np.array([int((grade[sb[s]:sb[s + 1]] >= binp).sum()) for s in range(nq)], np.int32)
    lg = np.log2(1.0 + np.arange(max(ncut) + 1, dtype=np.float64))
    idcg = np.zeros((nq, len(ncut)))
    for s in range(nq):
        best = np.sort(np.maximum(grade[sb[s]:sb[s + 1]].astype(np.int64), 0))[::-1]
        for c, cut in enumerate(ncut):
            idcg[s, c] = sum(g_ / lg[r + 1] for r, g_ in enumerate(best[:cut]))
    want = RR.rank_ref(torch.from_numpy(scores).to(dtype).float().numpy(), sb)
    rest = (binp, rcut, ncut, map_cut, bnr, idcg, lg)
    devs = dict(scores=_t(scores, dev, dtype), sb=_t(sb, dev), grade=_t(grade, dev), cand_pos=_t(cand_pos, dev), bnr=_t(bnr, dev),
                idcg=_t(idcg, dev), lg=_t(lg, dev))
    return dict(sb=sb, n=n, grade=grade, cand_pos=cand_pos, rest=rest, want=want, dev=devs, max_len=max(lengths))


def _check_metrics(got, ref):
    """tests/test_rank_metrics_gpu.py::_check_form: first_rank and hits exactly, AP and nDCG within 2 (m + 1) u |want|"""
    from tests import rank_metrics_reference as RR
    m = ref[4]
    shape1 = m.reshape(m.shape + (1,) * (ref[2].ndim - 1))
    assert np.array_equal(_np(got[0]), ref[0]) and np.array_equal(_np(got[1]), ref[1])
    RR.assert_close(_np(got[2]), ref[2], shape1, "ap")
    RR.assert_close(_np(got[3]), ref[3], shape1[..., None], "ndcg")


def _rank_stage(dev, dtype, chain):
    from matchmaker_amd import ops
    from tests import rank_metrics_reference as RR
    r = _rank_setup(dev, dtype)
    v = r["dev"]
    binp, rcut, ncut, map_cut = r["rest"][:4]

    def check(out):          # tests/test_rank_metrics_gpu.py::_check_order
        assert out.dtype == torch.int32 and np.array_equal(_np(out), r["want"])
    st = {"run": lambda: ops.segment_rank(v["scores"], v["sb"], r["max_len"]), "check": check}

    def consumer(order):
        tail = (binp, rcut, ncut, map_cut, v["bnr"], v["idcg"], v["lg"])
        o = _np(order)
        hi = r["max_len"]
        return [
            {"name": "rank_metrics-plain", "run": lambda: ops.rank_metrics(order, v["sb"], v["grade"], None, 2 ** 31 - 1, *tail),
             "check": lambda got: _check_metrics(got, RR.metrics_ref(o, r["sb"], r["grade"], None, RR.I32_MAX, *r["rest"]))},
            {"name": "rank_metrics-threshold-10", "run": lambda: ops.rank_metrics(order, v["sb"], v["grade"], v["cand_pos"], 10, *tail),
             "check": lambda got: _check_metrics(got, RR.metrics_ref(o, r["sb"], r["grade"], r["cand_pos"], 10, *r["rest"]))},
            {"name": "rank_metrics_depth", "run": lambda: ops.rank_metrics_depth(order, v["sb"], v["grade"], v["cand_pos"], hi, *tail),
             "check": lambda got: _check_metrics(got, RR.depth_ref(o, r["sb"], r["grade"], r["cand_pos"], hi, *r["rest"]))}]
    if chain:
        st["ints"] = lambda out: [("order", out, 0, r["n"])]
        st["next"] = consumer
    return st


case("segment_rank-f32", "segment_rank")(lambda dev: _rank_stage(dev, torch.float32, False))
case("segment_rank-bf16", "segment_rank")(lambda dev: _rank_stage(dev, torch.bfloat16, False))
case("chain-segment_rank->rank_metrics+rank_metrics_depth", "segment_rank", "rank_metrics", "rank_metrics_depth")(
    lambda dev: _rank_stage(dev, torch.float32, True))


# ======================================================================================================= the test
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_poisoned(c):
    dev = util.require_gpu()
    st = c.build(dev)
    _drive([st, st], c.name)



# ======================================================================================================= pooling-backward twins
TWIN_SHAPES = [(4, 20, 200, 300), (3, 30, 47, 64)]
TWINS = {"f32": {"MM_KP_BWD_F32": "1"}, "f32-512-threads": {"MM_KP_BWD_F32": "1", "MM_KP_BWD_THREADS": "512"},
         "untiled": {"MM_KP_BWD_UNTILED": "1"}, "nsplit1": {"MM_KP_BWD_NSPLIT": "1"}, "nsplit2": {"MM_KP_BWD_NSPLIT": "2"},
         "nsplit8": {"MM_KP_BWD_NSPLIT": "8"}}
TWIN_ENV = sorted({k for env in TWINS.values() for k in env})


def _twin_results(dev):
    """{(shape, gated): (inputs, [poisoned-run gradients])}: the poisoned pooling-backward case at the twins' two shapes"""
    res = {}
    for shape in TWIN_SHAPES:
        for gated in (False, True):
            x = pool_inputs(*shape, 11, gated, seed=sum(shape) + gated)
            st = _pool_bwd_stage(x, _pool_dev(x, dev))
            outs = [poison.run(st["run"], p, label=f"twin {shape} gated={gated} [{p:#04x}]")[0] for p in poison.POISONS]
            poison.assert_same_bits(outs[0], outs[1], f"twin {shape} gated={gated}")
            st["check"](outs[0])                  # fp64 autograd at the tolerances of test_kernel_pool_gpu.py / test_variants_gpu.py
            res[shape, gated] = outs[0]
    return res


def run_twin(label, default_npz):
    """In the child (the switches of `label` are in its environment): the poisoned case on this process's kernels, and for the
    exact-f32 settings the comparison with the default split kernel's gradients, atol 4e-4 x scale, rtol 4e-3 (the bound
    tests/test_kernel_pool_gpu.py states for two backward kernels of one input)."""
    dev = util.require_gpu()
    res = _twin_results(dev)
    if label.startswith("f32"):
        default = np.load(default_npz)
        for (shape, gated), got in res.items():
            for i, g_ in enumerate(got):
                want = default["{}-{}-{}-{}".format(*shape) + f"-{int(gated)}-{i}"]
                scale = max(1.0, float(np.abs(want).max()))
                np.testing.assert_allclose(_np(g_), want, atol=4e-4 * scale, rtol=4e-3, err_msg=f"{label} {shape} gated={gated} output {i}")
    print(f"twin {label}: {len(res)} cases ok")


@functools.lru_cache(maxsize=None)
def _default_results(path):
    assert not any(os.environ.get(k) for k in TWIN_ENV), "the parent runs the default kernels"
    res = _twin_results(util.require_gpu())
    np.savez(path, **{"{}-{}-{}-{}".format(*shape) + f"-{int(gated)}-{i}": _np(g_)
                      for (shape, gated), got in res.items() for i, g_ in enumerate(got)})
    return path


@pytest.mark.parametrize("label", list(TWINS))
def test_pooling_backward_twins_write_all_they_own(label, tmp_path_factory):
    """One fresh child per setting (tests/test_zz_rank_order_gpu.py's _child pattern; never an exec of this process)."""
    path = _default_results(str(tmp_path_factory.getbasetemp() / "kp_bwd_default.npz"))
    env = {k: v for k, v in os.environ.items() if k not in TWIN_ENV}
    r = subprocess.run([sys.executable, "-c", f"from tests.test_poisoned_memory_gpu import run_twin; run_twin({label!r}, {path!r})"],
                       cwd=ROOT, env=dict(env, **TWINS[label]), capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
