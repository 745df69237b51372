"""CPU: the float64 restatement of the all-pairs MaxSim backward equals autograd through oracle.torch_port.maxsim_inbatch;
the new C symbols are declared, bound and exported; the registered ops have a fake rule and maxsim_inbatch has a backward."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_port as TP
from tests import maxsim_inbatch_bwd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(Bq, Bd, Q=13, D=47, E=16, seed=0):
    g = np.random.default_rng(seed)
    q = g.standard_normal((Bq, Q, E))
    d = g.standard_normal((Bd, D, E))
    qm = np.ones((Bq, Q), dtype=np.int64)
    dm = np.ones((Bd, D), dtype=np.int64)
    qm[0, 9:] = 0                    # a padded query tail
    qm[1, 4] = 0                     # a hole in the query mask
    qm[Bq - 1, :] = 0                # one fully padded query token row
    dm[0, 30:] = 0                   # a padded document tail
    dm[1, 7] = 0                     # a hole in a document mask
    dm[1, 20:23] = 0
    dm[Bd - 1, :] = 0                # one fully padded document
    d[2, 40] = d[2, 3]               # equal rows far apart: the first takes the gradient
    go = g.standard_normal((Bq, Bd))
    return q, qm, d, dm, go


@pytest.mark.parametrize("Bq,Bd,bug", [(3, 5, False), (4, 4, True), (4, 4, False)])
def test_restatement_equals_fp64_autograd_through_the_torch_port(Bq, Bd, bug):
    q, qm, d, dm, go = _case(Bq, Bd)
    tq = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    td = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    out = TP.maxsim_inbatch(tq, torch.tensor(qm), td, torch.tensor(dm), bug_compatible=bug)
    out.backward(torch.tensor(go))
    ref = R.gradients(q, qm, d, dm, go, bug)
    assert np.abs(ref["gq"] - tq.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["gd"] - td.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["gq"]).max() > 0 and np.abs(ref["gd"]).max() > 0
    # what was planted: nothing flows into the padded query row, the padded document, masked positions; the first of two
    # equal rows takes all of it
    assert not ref["gq"][Bq - 1].any() and not ref["gq"][0, 9:].any() and not ref["gq"][1, 4].any()
    assert (ref["table"][:, 2] != 40).all()
    if not bug:
        assert not ref["gd"][Bd - 1].any() and not ref["gd"][1, 7].any() and not ref["gd"][0, 30:].any()
        assert (ref["table"][:, Bd - 1] == -1).all()
    else:
        assert (ref["table"][Bq - 1] == -1).all()          # row i's mask: query 3 sees every document fully padded
    # the terms per element add up to the cells that carry a gradient, on both sides
    assert ref["nq"].sum() == (ref["table"] >= 0).sum() == ref["nd"].sum()


def test_bug_compatible_restatement_needs_a_square_batch():
    q, qm, d, dm, go = _case(3, 5)
    with pytest.raises(ValueError):
        R.gradients(q, qm, d, dm, go, True)


def test_first_position_wins_exact_ties():
    q = np.ones((1, 1, 4))
    d = np.zeros((1, 6, 4))
    d[0, 2] = d[0, 5] = 0.5
    ref = R.gradients(q, np.ones((1, 1)), d, np.ones((1, 6)), np.ones((1, 1)))
    assert ref["table"][0, 0, 0] == 2 and ref["gd"][0, 2].all() and not ref["gd"][0, 5].any()
    gap, mx = R.min_gap(q, np.ones((1, 1)), d, np.ones((1, 6)))
    assert gap == 0.0 and mx == 2.0


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from matchmaker_amd import _lib
    from tests import abi
    L = abi.assert_bound(("mm_maxsim_inbatch_bwd_workspace_bytes", "mm_maxsim_inbatch_bwd"))
    hdr = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    assert "colbert.py:154-162" in hdr and "train.py:434-467" in hdr and "503-524" in hdr
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    # the size query is host arithmetic: masks + the int16 [Bq, Bd, Q] arg-max table
    none = L.mm_maxsim_inbatch_bwd_workspace_bytes(32, 64, 32, 180, 128, _lib.MASK_NONE, _lib.MASK_LEN_I32)
    assert none >= 32 * 64 * 32 * 2
    assert L.mm_maxsim_inbatch_bwd_workspace_bytes(32, 64, 32, 180, 128, _lib.MASK_I64, _lib.MASK_I64) > none


def test_fake_rules_of_the_forward_and_the_backward_op():
    import matchmaker_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            q = torch.empty(4, 32, 128, dtype=dt, device="cuda")
            d = torch.empty(7, 180, 128, dtype=dt, device="cuda")
            go = torch.empty(4, 7, device="cuda")
            gq, gd = torch.ops.mm_native.maxsim_inbatch_backward(q, None, d, None, go, False)
            assert gq.shape == q.shape and gd.shape == d.shape and gq.dtype == dt and gd.dtype == dt
            gq, gd = torch.ops.mm_native.maxsim_inbatch_backward(q, None, d, None, go, False, True, False)
            assert gq.shape == q.shape and gd.numel() == 0 and gd.dtype == dt          # a gradient that is not needed: empty
    assert len(torch.ops.mm_native.maxsim_inbatch.default._schema.arguments) == 7
    assert len(torch.ops.mm_native.maxsim_inbatch_backward.default._schema.returns) == 2


def test_maxsim_inbatch_has_a_registered_backward():
    """Fails without the feature: every custom op gets an autograd kernel, so the forward's output had a grad_fn all along, but
    without a registered formula backward() raised "no autograd formula was registered".  On meta tensors no kernel runs and the
    autograd engine needs no device: the backward reaches the fake rule of mm_native::maxsim_inbatch_backward."""
    import matchmaker_amd.torch_ops  # noqa: F401
    for dt in (torch.bfloat16, torch.float32):
        q = torch.empty(2, 8, 16, dtype=dt, device="meta", requires_grad=True)
        d = torch.empty(3, 9, 16, dtype=dt, device="meta", requires_grad=True)
        s = torch.ops.mm_native.maxsim_inbatch(q, None, d, None, False)
        assert s.requires_grad and s.shape == (2, 3) and s.dtype == torch.float32
        s.backward(torch.empty(2, 3, device="meta"))
        assert q.grad.shape == q.shape and q.grad.dtype == dt and d.grad.shape == d.shape and d.grad.dtype == dt
    # one side frozen: its gradient is neither computed nor handed back
    q = torch.empty(2, 8, 16, device="meta", requires_grad=True)
    d = torch.empty(3, 9, 16, device="meta")
    gq, = torch.autograd.grad(torch.ops.mm_native.maxsim_inbatch(q, None, d, None, False), q, torch.empty(2, 3, device="meta"))
    assert gq.shape == q.shape and gq.dtype == torch.float32 and d.grad is None
