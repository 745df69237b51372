"""GPU: backward of the all-pairs MaxSim (mm_maxsim_inbatch_bwd) against the float64 restatement in
tests/maxsim_inbatch_bwd_reference.py: bit-equal on exact-arithmetic inputs, within a derived bound on random ones,
deterministic, fully written, and reachable through torch.ops.mm_native.maxsim_inbatch and ColBERT.

Exact arithmetic: token values k / 8 (|k| <= 4) and grad_out in {+-1, +-0.5, +-2} make every dot product a multiple of 1/64 below
2^24 / 64 and every gradient sum a multiple of 1/16 far below 2^24 / 16: exact in fp32 in any order, so the only freedom left is
the arg-max rule, and the float64 restatement cast to the gradient dtype is the one right answer.

Random data: the inputs are plain seeded randn draws, rounded to the dtype under test.  The seed of each (shape, dtype) was
searched on the CPU (the first seed from 0 upwards, about one in 3,000 at the larger shape) so that every decided cell's top-two
gap exceeds 64 E 2^-24 max|sim|: a condition on the inputs, asserted at the start of the test; no cell is excluded.
The per-element bound is (n + 2) 2^-24 sum|terms| + u_out |ref64|, plus 2^-25 for fp16 gradient elements with |ref64| < 2^-14:
fp16 is subnormal there, and without that term the correctly rounded float64 gradient itself misses the bound at 48 elements of
the larger shape.
"""
import functools

import numpy as np
import pytest
import torch

from tests import maxsim_inbatch_bwd_reference as R
from tests import util

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
U_OUT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float32: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}      # fp16 underflow: see maxsim_inbatch_bwd_reference.bound


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_bits(got, ref64, what):
    exp = torch.from_numpy(np.ascontiguousarray(ref64)).to(torch.float32).to(got.dtype)
    same = torch.equal(_bits(got.cpu()), _bits(exp))
    assert same, f"{what}: {int((_bits(got.cpu()) != _bits(exp)).sum())} elements differ in bits"


# --------------------------------------------------------------------------------------------- exact-arithmetic cases
@functools.lru_cache(maxsize=None)
def _exact_case(Bq, Bd, Q, D, E, bug):
    g = torch.Generator().manual_seed(1000 * Bq + 10 * Bd + Q + D + E)
    q = torch.randint(-4, 5, (Bq, Q, E), generator=g).double() / 8
    d = torch.randint(-4, 5, (Bd, D, E), generator=g).double() / 8
    go = torch.tensor([1.0, -1.0, 0.5, -0.5, 2.0, -2.0])[torch.randint(0, 6, (Bq, Bd), generator=g)].double()
    pat = (torch.randint(0, 2, (E,), generator=g).double() - 0.5)          # +-0.5 everywhere: <pat, pat> = E / 4 is the largest dot product
    p1, p2 = 2, D - 3
    d[0, p1] = pat
    d[0, p2] = pat                   # equal rows far apart: the first takes all the gradient, the second exactly none
    d[1, p1] = pat
    d[1, p2] = pat                   # ... and with a hole over the first one the second takes it
    q[:, 0] = pat                    # the same document row is the arg-max of a token of EVERY query
    q[:, 1] = pat
    qm = torch.ones(Bq, Q, dtype=torch.int64)
    dm = torch.ones(Bd, D, dtype=torch.int64)
    dm[1, p1] = 0                    # a mask hole
    dm[1, D // 2] = 0
    dm[0, D - 2:] = 0                # a padded tail
    dm[Bd - 1] = 0                   # a fully padded document
    qm[0, Q - 3:] = 0                # a padded query tail
    qm[Bq - 1, 3] = 0                # a hole in a query mask
    ref = R.gradients(q.numpy(), qm.numpy(), d.numpy(), dm.numpy(), go.numpy(), bug)
    return q, qm, d, dm, go, ref, (p1, p2)


EXACT_SHAPES = [(3, 5, 13, 47, 64), (4, 4, 40, 70, 24), (2, 9, 32, 180, 128), (2, 3, 8, 33, 768)]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bug", [False, True], ids=["own-mask", "bug-compatible"])
def test_exact_arithmetic_inputs_are_bit_equal_to_the_restatement(shape, dt, bug):
    from matchmaker_amd import _lib, ops
    dev = util.require_gpu()
    Bq, Bd = shape[:2]
    if bug and Bq != Bd:
        q, qm, d, dm, go, _, _ = _exact_case(*shape, False)
        with pytest.raises(ops.NativeError) as e:
            ops.maxsim_inbatch_bwd(q.to(dev, dt), qm.to(dev), d.to(dev, dt), dm.to(dev), go.to(dev), bug_compatible=True)
        assert e.value.code == _lib.MM_EINVAL
        return
    q, qm, d, dm, go, ref, (p1, p2) = _exact_case(*shape, bug)
    for gdt in ([torch.float32] if dt == torch.float32 else [torch.float32, dt]):
        gq, gd = ops.maxsim_inbatch_bwd(q.to(dev, dt), qm.to(dev), d.to(dev, dt), dm.to(dev), go.to(dev),
                                        bug_compatible=bug, grad_dtype=gdt)
        assert gq.dtype == gdt and gd.dtype == gdt and gq.shape == q.shape and gd.shape == d.shape
        _assert_bits(gq, ref["gq"], f"grad_q {gdt}")
        _assert_bits(gd, ref["gd"], f"grad_d {gdt}")
    if not bug:
        assert (ref["table"][:, 0, 0] == p1).all() and (ref["table"][1:, 1, 0] == p2).all()
        assert gd[0, p1].float().abs().sum() > 0 and not gd[0, p2].any() and not gd[1, p1].any()
        assert gd[1, p2].float().abs().sum() > 0 and not gd[Bd - 1].any() and not gq[0, shape[2] - 3:].any()


def test_the_raw_abi_refuses_bug_compatible_masking_of_a_non_square_batch():
    from matchmaker_amd import _lib
    dev = util.require_gpu()
    L = _lib.lib()
    q = torch.zeros(3, 8, 16, device=dev)
    d = torch.zeros(5, 9, 16, device=dev)
    go = torch.zeros(3, 5, device=dev)
    gq, gd = torch.empty_like(q), torch.empty_like(d)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    rc = L.mm_maxsim_inbatch_bwd(q.data_ptr(), d.data_ptr(), None, 0, None, 0, go.data_ptr(), gq.data_ptr(), gd.data_ptr(), 0,
                                 3, 5, 8, 9, 16, 0, 1, ws.data_ptr(), ws.numel(), 0)
    assert rc == _lib.MM_EINVAL and b"Bq == Bd" in L.mm_last_error()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_every_mask_encoding_gives_the_same_bits(dt):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    Bq, Bd, Q, D, E = 3, 4, 13, 47, 64
    q, _, d, _, go, _, _ = _exact_case(3, 5, Q, D, E, False)
    d, go = d[:Bd], go[:, :Bd]
    ql, dl = torch.tensor([13, 9, 1]), torch.tensor([47, 20, 33, 0])
    qm = (torch.arange(Q)[None] < ql[:, None])
    dm = (torch.arange(D)[None] < dl[:, None])
    ref = R.gradients(q.numpy(), qm.numpy(), d.numpy(), dm.numpy(), go.numpy())
    args = lambda a, b: ops.maxsim_inbatch_bwd(q.to(dev, dt), a, d.to(dev, dt), b, go.to(dev))
    for enc in (lambda m, l: l.to(dev), lambda m, l: l.to(dev, torch.int32), lambda m, l: m.to(dev), lambda m, l: m.to(dev, torch.uint8),
                lambda m, l: m.to(dev, torch.int64), lambda m, l: m.to(dev, torch.float32)):
        gq, gd = args(enc(qm, ql), enc(dm, dl))
        _assert_bits(gq, ref["gq"], "grad_q")
        _assert_bits(gd, ref["gd"], "grad_d")
    ones = R.gradients(q.numpy(), np.ones((Bq, Q)), d.numpy(), np.ones((Bd, D)), go.numpy())
    gq, gd = args(None, None)
    _assert_bits(gq, ones["gq"], "grad_q without masks")
    _assert_bits(gd, ones["gd"], "grad_d without masks")


# --------------------------------------------------------------------------------------------- random data
def _threshold(E, mx):
    return 64 * E * 2.0 ** -24 * mx


# first seed from 0 upwards whose plain draw meets the input condition (searched on the CPU in float64 on the rounded inputs)
SEEDS = {((6, 10, 32, 180, 128), torch.bfloat16): 4236, ((6, 10, 32, 180, 128), torch.float16): 943,
         ((6, 10, 32, 180, 128), torch.float32): 943,
         ((5, 3, 13, 47, 64), torch.bfloat16): 0, ((5, 3, 13, 47, 64), torch.float16): 0, ((5, 3, 13, 47, 64), torch.float32): 0}


@functools.lru_cache(maxsize=None)
def _random_case(Bq, Bd, Q, D, E, dt):
    """Seeded randn rounded to `dt` (queries scaled by E^-0.5), mixed lengths incl. one fully padded document and a mask hole."""
    g = torch.Generator().manual_seed(SEEDS[(Bq, Bd, Q, D, E), dt])
    q = (torch.randn(Bq, Q, E, generator=g) * E ** -0.5).to(dt)
    d = torch.randn(Bd, D, E, generator=g).to(dt)
    go = torch.randn(Bq, Bd, generator=g)
    ql = torch.randint(Q // 2, Q + 1, (Bq,), generator=g)
    dl = torch.randint(D // 3, D + 1, (Bd,), generator=g)
    dl[0], dl[Bd - 1] = D, 0
    qm = (torch.arange(Q)[None] < ql[:, None]).long()
    dm = (torch.arange(D)[None] < dl[:, None]).long()
    dm[1, 5] = 0
    ref = R.gradients(q.double().numpy(), qm.numpy(), d.double().numpy(), dm.numpy(), go.double().numpy())
    return q, qm, d, dm, go, ref


def _assert_condition(q, qm, d, dm, E):
    gap, mx = R.min_gap(q.double().numpy(), qm.numpy(), d.double().numpy(), dm.numpy())
    assert gap > _threshold(E, mx), f"input condition: smallest top-two gap {gap:.3e} <= {_threshold(E, mx):.3e}"


def _assert_within_bound(got, ref, terms, n, gdt, what):
    err = np.abs(got.double().cpu().numpy() - ref)
    bnd = R.bound(ref, terms, n, U_OUT[gdt], TINY[gdt])
    worst = float((err - bnd).max())
    print(f"{what}: max err {err.max():.3e}, max err / bound {float((err / np.maximum(bnd, 1e-300)).max()):.3f}")
    assert worst <= 0, f"{what}: |got - ref64| exceeds the bound by {worst:.3e} ({int((err > bnd).sum())} elements)"


RANDOM_SHAPES = [(6, 10, 32, 180, 128), (5, 3, 13, 47, 64)]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_data_is_within_the_derived_bound_of_fp64(shape, dt):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, qm, d, dm, go, ref = _random_case(*shape, dt)
    _assert_condition(q, qm, d, dm, shape[4])
    for gdt in ([torch.float32] if dt == torch.float32 else [torch.float32, dt]):
        gq, gd = ops.maxsim_inbatch_bwd(q.to(dev), qm.to(dev), d.to(dev), dm.to(dev), go.to(dev), grad_dtype=gdt)
        _assert_within_bound(gq, ref["gq"], ref["aq"], ref["nq"], gdt, f"grad_q {dt}->{gdt}")
        _assert_within_bound(gd, ref["gd"], ref["ad"], ref["nd"], gdt, f"grad_d {dt}->{gdt}")


# --------------------------------------------------------------------------------------------- determinism, full write
def _raw_call(q, qm, d, dm, go, gq, gd, bug=False):
    from matchmaker_amd import _lib, ops
    L = _lib.lib()
    Bq, Q, E = q.shape
    Bd, D, _ = d.shape
    wsb = L.mm_maxsim_inbatch_bwd_workspace_bytes(Bq, Bd, Q, D, E, _lib.MASK_I64, _lib.MASK_I64)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    rc = L.mm_maxsim_inbatch_bwd(q.data_ptr(), d.data_ptr(), qm.data_ptr(), _lib.MASK_I64, dm.data_ptr(), _lib.MASK_I64,
                                 go.data_ptr(), gq.data_ptr(), gd.data_ptr(), ops._DT[gq.dtype], Bq, Bd, Q, D, E, ops._DT[q.dtype],
                                 1 if bug else 0, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mm_maxsim_inbatch_bwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt,gdt", [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32), (torch.float32, torch.float32)],
                         ids=["bf16-bf16", "fp16-f32", "f32-f32"])
def test_two_calls_are_bit_equal_and_every_byte_is_written(dt, gdt):
    dev = util.require_gpu()
    q, qm, d, dm, go, _ = _random_case(6, 10, 32, 180, 128, dt)
    q, qm, d, dm, go = q.to(dev), qm.to(dev), d.to(dev), dm.to(dev), go.to(dev)
    outs = []
    for _ in range(2):
        gq = torch.full(q.shape, float("nan"), dtype=gdt, device=dev)
        gd = torch.full(d.shape, float("nan"), dtype=gdt, device=dev)
        _raw_call(q, qm, d, dm, go, gq, gd)
        assert not torch.isnan(gq).any() and not torch.isnan(gd).any()
        outs.append((gq, gd))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    gd = outs[0][1]
    assert torch.equal(_bits(gd[-1]), torch.zeros_like(_bits(gd[-1])))          # the fully padded document: exactly +0
    assert gd[:-1].float().abs().sum() > 0 and outs[0][0].float().abs().sum() > 0


# --------------------------------------------------------------------------------------------- large tile
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_a_document_too_long_for_a_full_width_accumulator_is_tiled_over_columns(dt):
    """D E 4 = 1.8 MB: the per-document accumulator narrows to 23 columns per workgroup; same bits as the restatement."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, qm, d, dm, go, ref, _ = _exact_case(2, 2, 8, 600, 768, False)
    gq, gd = ops.maxsim_inbatch_bwd(q.to(dev, dt), qm.to(dev), d.to(dev, dt), dm.to(dev), go.to(dev))
    _assert_bits(gq, ref["gq"], "grad_q")
    _assert_bits(gd, ref["gd"], "grad_d")


# --------------------------------------------------------------------------------------------- public surface
def test_the_registered_op_is_differentiable_and_its_backward_is_the_native_one():
    """Fails without the feature: backward() raised "no autograd formula was registered"."""
    import matchmaker_amd.torch_ops  # noqa: F401
    from matchmaker_amd import ops
    dev = util.require_gpu()
    for dt in (torch.bfloat16, torch.float32):
        q, qm, d, dm, go, _ = _random_case(5, 3, 13, 47, 64, dt)
        q, qm, d, dm, go = q.to(dev).requires_grad_(), qm.to(dev), d.to(dev).requires_grad_(), dm.to(dev), go.to(dev)
        s = torch.ops.mm_native.maxsim_inbatch(q, qm, d, dm, False)
        assert s.requires_grad and s.grad_fn is not None
        assert torch.equal(s.detach(), ops.maxsim_inbatch(q.detach(), qm, d.detach(), dm))
        s.backward(go)
        gq, gd = ops.maxsim_inbatch_bwd(q.detach(), qm, d.detach(), dm, go, grad_dtype=dt)
        assert q.grad.dtype == dt and d.grad.dtype == dt
        assert torch.equal(_bits(q.grad), _bits(gq)) and torch.equal(_bits(d.grad), _bits(gd))
    # only one side requires grad: the other side's pass is not run, the wanted gradient has the same bits
    q2, d2 = q.detach().clone().requires_grad_(), d.detach().clone()
    torch.ops.mm_native.maxsim_inbatch(q2, qm, d2, dm, False).backward(go)
    assert torch.equal(_bits(q2.grad), _bits(gq)) and d2.grad is None
    q3, d3 = q.detach().clone(), d.detach().clone().requires_grad_()
    torch.ops.mm_native.maxsim_inbatch(q3, qm, d3, dm, False).backward(go)
    assert torch.equal(_bits(d3.grad), _bits(gd)) and q3.grad is None
    oq, none = ops.maxsim_inbatch_bwd(q3, qm, d2, dm, go, grad_dtype=dt, need_d=False)
    none2, od = ops.maxsim_inbatch_bwd(q3, qm, d2, dm, go, grad_dtype=dt, need_q=False)
    assert none is None and none2 is None and torch.equal(_bits(oq), _bits(gq)) and torch.equal(_bits(od), _bits(gd))


def test_autocast_hands_fp32_leaves_fp32_gradients_of_the_fp16_vectors():
    import matchmaker_amd.torch_ops  # noqa: F401
    dev = util.require_gpu()
    shape = (5, 3, 13, 47, 64)
    q16, qm, d16, dm, go, ref = _random_case(*shape, torch.float16)
    _assert_condition(q16, qm, d16, dm, shape[4])
    q = q16.float().to(dev).requires_grad_()          # fp32 leaves whose fp16 cast is exact: the backward sees q16, d16
    d = d16.float().to(dev).requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        s = torch.ops.mm_native.maxsim_inbatch(q, qm.to(dev), d, dm.to(dev), False)
    assert s.dtype == torch.float32
    s.backward(go.to(dev))
    assert q.grad.dtype == torch.float32 and d.grad.dtype == torch.float32
    # the native gradient is rounded once to fp16 (the cast vectors' dtype); the cast node's fp16 -> fp32 is exact
    _assert_within_bound(q.grad, ref["gq"], ref["aq"], ref["nq"], torch.float16, "autocast grad_q")
    _assert_within_bound(d.grad, ref["gd"], ref["ad"], ref["nd"], torch.float16, "autocast grad_d")


def _model(dev, dim=32):
    from transformers import BertConfig, BertModel
    from matchmaker_amd.colbert import ColBERT, ColBERTConfig
    torch.manual_seed(0)
    enc = BertModel(BertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                               vocab_size=500, max_position_embeddings=256))
    return ColBERT(ColBERTConfig(bert_model="(injected)", compression_dim=dim), bert_model=enc).to(dev).eval()


def _batch(dev, Bq=3, Bd=3, Q=8, D=12):
    g = torch.Generator().manual_seed(1)
    mk = lambda B, L, n: {"input_ids": torch.randint(1, 500, (B, n), generator=g).to(dev),
                          "attention_mask": (torch.arange(n)[None] < L[:, None]).long().to(dev)}
    return mk(Bq, torch.tensor([8, 5, 3][:Bq]), Q), mk(Bd, torch.tensor([12, 7, 9][:Bd]), D)


@pytest.mark.parametrize("bug", [False, True], ids=["own-mask", "bug-compatible"])
def test_colbert_inbatch_aggregation_backpropagates_into_the_compressor(bug):
    """Native path and eager autograd of the same module through torch_port.maxsim_inbatch, fp32.  Each is within the bound b of
    tests/maxsim_inbatch_bwd_reference.bound (u_out = 2^-24) of the exact gradient at the token vectors, so they differ by <= 2 b
    there; compressor.weight.grad[e, h] = sum_rows g[row, e] hidden[row, h] (R rows, an fp32 matrix product on both sides), hence
      |dW[e, h]| <= sum_rows 2 b[row, e] |hidden[row, h]| + 2 (R + 2) 2^-24 sum_rows |g[row, e]| |hidden[row, h]|."""
    from oracle import torch_port as TP
    dev = util.require_gpu()
    model = _model(dev)
    model.inbatch_bug_compatible = bug
    query, doc = _batch(dev)
    go = torch.tensor([[1.0, -0.5, 0.25], [-1.0, 2.0, 0.5], [0.75, -0.25, 1.5]], device=dev)

    def run(native):
        model.zero_grad()
        qv, dv = model.forward_representation(query), model.forward_representation(doc)
        qv.retain_grad()
        dv.retain_grad()
        if native:
            s = model.forward_inbatch_aggregation(qv, query["attention_mask"], dv, doc["attention_mask"])
        else:
            s = TP.maxsim_inbatch(qv, query["attention_mask"], dv, doc["attention_mask"], bug_compatible=bug)
        assert s.requires_grad
        s.backward(go)
        return s.detach(), qv.detach(), dv.detach(), qv.grad, dv.grad, model.compressor.weight.grad.clone()

    s_n, qv, dv, gq_n, gd_n, w_n = run(True)
    s_e, qv_e, dv_e, gq_e, gd_e, w_e = run(False)
    assert torch.equal(qv, qv_e) and torch.equal(dv, dv_e)
    qm, dm = query["attention_mask"].cpu().numpy(), doc["attention_mask"].cpu().numpy()
    gap, mx = R.min_gap(qv.double().cpu().numpy(), qm, dv.double().cpu().numpy(), dm, bug)
    assert gap > _threshold(qv.shape[-1], mx), f"input condition: gap {gap:.3e}"
    ref = R.gradients(qv.double().cpu().numpy(), qm, dv.double().cpu().numpy(), dm, go.double().cpu().numpy(), bug)
    _assert_within_bound(gq_n, ref["gq"], ref["aq"], ref["nq"], torch.float32, "ColBERT grad at query vectors")
    _assert_within_bound(gd_n, ref["gd"], ref["ad"], ref["nd"], torch.float32, "ColBERT grad at document vectors")
    with torch.no_grad():
        hq = model.bert_model(**query)[0].double().cpu().numpy().reshape(-1, 64)
        hd = model.bert_model(**doc)[0].double().cpu().numpy().reshape(-1, 64)
    E = qv.shape[-1]
    b = np.concatenate([R.bound(ref["gq"], ref["aq"], ref["nq"], 2.0 ** -24).reshape(-1, E),
                        R.bound(ref["gd"], ref["ad"], ref["nd"], 2.0 ** -24).reshape(-1, E)])
    gabs = np.abs(np.concatenate([ref["gq"].reshape(-1, E), ref["gd"].reshape(-1, E)]))
    habs = np.abs(np.concatenate([hq, hd]))
    rows = habs.shape[0]
    wb = 2 * b.T @ habs + 2 * (rows + 2) * 2.0 ** -24 * (gabs.T @ habs)
    werr = np.abs(w_n.double().cpu().numpy() - w_e.double().cpu().numpy())
    print(f"compressor.weight.grad: max |native - eager| {werr.max():.3e}, max err / bound {float((werr / np.maximum(wb, 1e-300)).max()):.3f}")
    assert w_n.abs().sum() > 0 and (werr <= wb).all()
    assert float((s_n - s_e).abs().max()) <= 1e-5 * (1 + float(s_e.abs().max()))

    # without a gradient the call takes the plain forward: bit-equal scores
    from matchmaker_amd import ops
    with torch.no_grad():
        s0 = model.forward_inbatch_aggregation(qv, query["attention_mask"], dv, doc["attention_mask"])
    plain = ops.maxsim_inbatch(qv, query["attention_mask"], dv, doc["attention_mask"], bug_compatible=bug)
    assert not s0.requires_grad and torch.equal(s0, plain) and torch.equal(s0, s_n)


def test_the_backward_call_replays_from_a_captured_graph_to_the_same_bits():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, qm, d, dm, go, _ = _random_case(5, 3, 13, 47, 64, torch.bfloat16)
    q, qm, d, dm, go = q.to(dev), qm.to(dev), d.to(dev), dm.to(dev), go.to(dev)
    eq, ed = ops.maxsim_inbatch_bwd(q, qm, d, dm, go, grad_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gq, gd = ops.maxsim_inbatch_bwd(q, qm, d, dm, go, grad_dtype=torch.bfloat16)
    gq.fill_(float("nan"))
    gd.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(gq), _bits(eq)) and torch.equal(_bits(gd), _bits(ed))


# --------------------------------------------------------------------------------------------- paired backward
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "f32"])
def test_a_diagonal_grad_out_reproduces_the_paired_backward(dt):
    """grad_out = diag(g) leaves the three diagonal pairs: the bits of ops.maxsim_bwd on them, except that an element may be -0
    there and +0 here: the paired kernel scales a single row, g x, and so writes -0 for a negative g and a zero x where a sum
    that starts from +0 gives +0.  Every element whose bits differ must be such a pair of zeros."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, qm, d, dm, go, _, _ = _exact_case(3, 5, 13, 47, 64, False)
    q, qm, d, dm = q.to(dev, dt), qm.to(dev), d[:3].to(dev, dt), dm[:3].to(dev)
    g = go[0, :3].float().to(dev)
    pq, pd = ops.maxsim_bwd(q, d, qm, dm, g, grad_dtype=dt)
    gq, gd = ops.maxsim_inbatch_bwd(q, qm, d, dm, torch.diag(g), grad_dtype=dt)
    for got, pair in ((gq, pq), (gd, pd)):
        differ = _bits(got) != _bits(pair)
        assert (got[differ] == 0).all() and (pair[differ] == 0).all(), "bits differ at an element that is not a +-0 pair"
    assert pq.float().abs().sum() > 0 and pd.float().abs().sum() > 0
