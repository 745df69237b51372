"""CPU tests of MatchPyramid's native backward (no GPU): the ABI symbols, the fake (meta) rules of
torch.ops.mm_native.matchpyramid_features_train and its backward op, the host operators' argument checks, the envelope
checks of the C entry points (they return before any launch), and the oracles of tests/matchpyramid_bwd_reference.py against
each other: the given-arg-max form fed torch's own return_indices IS the module's backward, bit for bit in fp64, and the
inputs of the direct comparison are decided (every strict gap above twice the forward tolerance) before the GPU test uses
them."""
import ctypes

import pytest
import torch

from tests import matchpyramid_bwd_reference as BR
from tests import matchpyramid_reference as MR

NEW = ("mm_matchpyramid_fwd_save_workspace_bytes", "mm_matchpyramid_fwd_save", "mm_matchpyramid_bwd_workspace_bytes",
       "mm_matchpyramid_bwd")


def _arr(channels, kernels, pools):
    rows = [x for c, k, p in zip(channels, kernels, pools) for x in (c, k[0], k[1], p[0], p[1])]
    return (ctypes.c_int32 * len(rows))(*rows)


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from matchmaker_amd import _lib
    from tests import abi
    L = abi.assert_bound(NEW)
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    arr = _arr(*MR.DEFAULT)
    one = L.mm_matchpyramid_bwd_workspace_bytes(1, 30, 200, 5, arr)
    assert 0 < one < 4 << 20
    assert L.mm_matchpyramid_bwd_workspace_bytes(10 ** 6, 30, 200, 5, arr) <= 256 << 20     # bounded however large the batch
    assert L.mm_matchpyramid_fwd_save_workspace_bytes(10 ** 6, 30, 200, 5, arr) <= 256 << 20
    assert L.mm_matchpyramid_fwd_save_workspace_bytes(1, 30, 200, 5, arr) == (16 * 38 * 92 + 16) * 4   # as the forward's
    assert L.mm_matchpyramid_bwd_workspace_bytes(4, 65, 200, 5, arr) == 0


# one step past every limit of the forward's envelope: (Q, D, E, channels, kernels, pools)
REFUSED = [
    (65, 20, 16, [4], [[3, 3]], [[2, 2]]),
    (8, 2049, 16, [4], [[3, 3]], [[2, 2]]),
    (8, 20, 1028, [4], [[3, 3]], [[2, 2]]),
    (8, 20, 18, [4], [[3, 3]], [[2, 2]]),
    (8, 20, 16, [4] * 9, [[3, 3]] * 9, [[2, 2]] * 9),
    (8, 20, 16, [33], [[3, 3]], [[2, 2]]),
    (8, 20, 16, [4], [[6, 3]], [[2, 2]]),
    (8, 20, 16, [4], [[3, 6]], [[2, 2]]),
    (8, 20, 16, [4], [[3, 3]], [[65, 2]]),
    (8, 20, 16, [4], [[3, 3]], [[2, 257]]),
    (2, 20, 16, [4], [[5, 1]], [[2, 2]]),
]


@pytest.mark.parametrize("Q, D, E, channels, kernels, pools", REFUSED)
def test_one_past_each_limit_is_refused_before_any_launch(Q, D, E, channels, kernels, pools):
    """host memory for every pointer and n_pairs = 0: nothing is dereferenced, nothing is launched"""
    from matchmaker_amd import _lib
    L = _lib.lib()
    arr = _arr(channels, kernels, pools)
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = len(channels)
    assert L.mm_matchpyramid_fwd_save(p, p, p, p, p, p, p, 0, 1, Q, D, E, n, arr, None, 0, None) == _lib.MM_EUNSUPPORTED
    assert L.mm_matchpyramid_bwd(p, p, p, p, p, p, p, p, p, p, 0, 1, Q, D, E, n, arr, None, 0, None) == _lib.MM_EUNSUPPORTED
    assert L.mm_matchpyramid_bwd_workspace_bytes(2, Q, D, n, arr) == 0 or E != 16
    assert L.mm_matchpyramid_fwd_save_workspace_bytes(2, Q, D, n, arr) == 0 or E != 16


def test_null_pointers_bad_counts_and_the_empty_batch():
    from matchmaker_amd import _lib
    L = _lib.lib()
    arr = _arr(*MR.DEFAULT)
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    shape = (30, 200, 64, 5, arr, None, 0, None)
    for k in range(7):                           # every pointer of the save entry
        a = [p] * 7
        a[k] = None
        assert L.mm_matchpyramid_fwd_save(*a, 2, 1, *shape) == _lib.MM_EINVAL
    for k in range(10):                          # every pointer of the backward
        a = [p] * 10
        a[k] = None
        assert L.mm_matchpyramid_bwd(*a, 2, 1, *shape) == _lib.MM_EINVAL
    assert L.mm_matchpyramid_fwd_save(*[p] * 7, 2, 1, 30, 200, 64, 5, None, None, 0, None) == _lib.MM_EINVAL
    assert L.mm_matchpyramid_bwd(*[p] * 10, 2, 1, 30, 200, 64, 5, None, None, 0, None) == _lib.MM_EINVAL
    assert L.mm_matchpyramid_fwd_save(*[p] * 7, 2, 0, *shape) == _lib.MM_EINVAL
    assert L.mm_matchpyramid_bwd(*[p] * 10, 2, 0, *shape) == _lib.MM_EINVAL
    assert L.mm_matchpyramid_fwd_save(*[p] * 7, 2, 1, *shape) == _lib.MM_EWORKSPACE
    assert L.mm_matchpyramid_bwd(*[p] * 10, 2, 1, *shape) == _lib.MM_EWORKSPACE
    assert L.mm_matchpyramid_fwd_save(*[p] * 7, 0, 1, *shape) == _lib.MM_OK
    assert L.mm_matchpyramid_bwd(*[p] * 10, 0, 1, *shape) == _lib.MM_OK


@pytest.mark.parametrize("nq, ppq, B", [(4, 1, 4), (2, 1000, 1500)])
def test_fake_tensor_shapes_forward_and_backward(nq, ppq, B):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from matchmaker_amd import torch_ops  # noqa: F401
    channels, kernels, pools = MR.DEFAULT
    flat = [x for p in pools for x in p]
    S = 16 * (36 * 90 + 18 * 60 + 9 * 30 + 6 * 20 + 3 * 10)

    def params(device, grad=False):
        cin, w, b = 1, [], []
        for c, k in zip(channels, kernels):
            w.append(torch.empty(c, cin, k[0], k[1], device=device, requires_grad=grad))
            b.append(torch.empty(c, device=device, requires_grad=grad))
            cin = c
        return w, b

    with FakeTensorMode():
        w, b = params("cuda")
        q, d = torch.empty(nq, 30, 300, device="cuda"), torch.empty(B, 200, 300, device="cuda")
        f, pooled, argmax = torch.ops.mm_native.matchpyramid_features_train(q, d, w, b, flat, ppq)
        assert tuple(f.shape) == (B, 16 * 3 * 10) and f.dtype == torch.float32
        assert tuple(pooled.shape) == (B, S) and pooled.dtype == torch.float32
        assert tuple(argmax.shape) == (B, S) and argmax.dtype == torch.int32
        gq, gd, gw, gb = torch.ops.mm_native.matchpyramid_features_train_backward(q, d, w, b, flat, pooled, argmax, f, ppq)
        assert gq.shape == q.shape and gd.shape == d.shape
        assert [t.shape for t in gw] == [t.shape for t in w] and [t.shape for t in gb] == [t.shape for t in b]
    w, b = params("meta", grad=True)
    q = torch.empty(nq, 30, 64, device="meta", requires_grad=True)
    d = torch.empty(B, 200, 64, device="meta", requires_grad=True)
    f, pooled, argmax = torch.ops.mm_native.matchpyramid_features_train(q, d, w, b, flat, ppq)
    assert f.requires_grad and not pooled.requires_grad and not argmax.requires_grad
    f.sum().backward()                           # the autograd formula runs on meta tensors: shapes and dtypes of every gradient
    assert q.grad.shape == q.shape and d.grad.shape == d.shape
    for t in w + b:
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype


def test_host_ops_reject_cpu_tensors_and_inconsistent_lists():
    from matchmaker_amd import ops, NativeError
    p = MR.random_params([4, 3], [[3, 3], [2, 2]], [[2, 2], [1, 2]], seed=1)
    w, b = MR.conv_lists(p)
    q, d = torch.zeros(1, 4, 16), torch.zeros(1, 9, 16)
    assert ops.matchpyramid_saved_size(w, p["pools"]) == 4 * 2 * 2 + 3 * 1 * 2
    saved = (torch.zeros(1, 22), torch.zeros(1, 22, dtype=torch.int32))
    with pytest.raises(NativeError, match="CPU tensor"):
        ops.matchpyramid_features_save(q, d, w, b, p["pools"])
    with pytest.raises(NativeError, match="CPU tensor"):
        ops.matchpyramid_bwd(q, d, w, b, p["pools"], saved, torch.zeros(1, 6))
    # the list checks both new operators make before anything else (the device check fires first on CPU tensors, so they
    # are reached directly; shapes of `saved` / `grad_features`: test_matchpyramid_bwd_gpu.py)
    for what in ("matchpyramid_features_save", "matchpyramid_bwd"):
        arr, feat = ops._mp_layers(4, 9, w, b, p["pools"], what)
        assert list(arr) == [4, 3, 3, 2, 2, 3, 2, 2, 1, 2] and feat == 3 * 1 * 2
        with pytest.raises(NativeError, match=what + ".*1 pool sizes"):
            ops._mp_layers(4, 9, w, b, p["pools"][:1], what)
        with pytest.raises(NativeError, match=what + ".*1 biases"):
            ops._mp_layers(4, 9, w, b[:1], p["pools"], what)
        with pytest.raises(NativeError, match=what + ".*after 4 channels"):
            ops._mp_layers(4, 9, [w[0], w[0]], b, p["pools"], what)
        with pytest.raises(NativeError, match=what + ".*bias"):
            ops._mp_layers(4, 9, w, [b[0], b[0]], p["pools"], what)
    with pytest.raises(NativeError, match="CPU tensor"):                  # an inconsistent list does not get past the device check
        ops.matchpyramid_bwd(q, d, w, b[:1], p["pools"], saved, torch.zeros(1, 6))


def test_module_switch_is_an_attribute_and_the_cpu_path_ignores_it():
    from matchmaker_amd.matchpyramid import MatchPyramid
    assert MatchPyramid.native_backward is False and "native_backward" in MatchPyramid.__doc__
    q, d, _, _ = BR.inputs("tiny")
    m = BR.module("tiny", torch.float32).train()
    a = m(q, d, None, None)
    m.native_backward = not MatchPyramid.native_backward
    assert "native_backward" in m.__dict__ and torch.equal(m(q, d, None, None), a)


@pytest.mark.parametrize("name", BR.DIRECT + ["zero"])
def test_given_argmax_form_with_torchs_indices_is_the_modules_backward_bit_for_bit(name):
    a = BR.oracle_a(name, torch.float64)
    b = BR.oracle_b(name, torch.float64, BR.planes(name, torch.float64)[1])
    assert torch.equal(a["features"], b["features"])
    assert torch.equal(a["gq"], b["gq"]) and torch.equal(a["gd"], b["gd"])
    for x, y in zip(a["gw"] + a["gb"], b["gw"] + b["gb"]):
        assert torch.equal(x, y)
    if name == "zero":                           # the case is what it says: exact ties above zero, zero rows with a gradient
        q, d, _, _ = BR.inputs(name)
        assert float(d[:, -3:].abs().max()) == 0 and float(q[:, 2].abs().max()) == 0
        assert any(bool(((cnt > 1) & (mx > 0)).any()) for mx, _, cnt in BR.element_gaps(name))
        assert torch.isfinite(a["gd"]).all() and float(a["gd"][:, -3:].abs().max()) > 1e6


@pytest.mark.parametrize("name", BR.DIRECT)
def test_direct_cases_are_decided_before_use(name):
    gap, t = BR.strict_gap_per_pair(name), BR.forward_tol(name)
    print(f"{name}: strict gap per pair = {[f'{x:.3e}' for x in gap.tolist()]}, forward tol = {t:.3e}")
    assert bool((gap > 2 * t).all())


def test_reference_config_is_not_decided_and_stays_out_of_the_direct_comparison():
    assert "ref" not in BR.DIRECT and "chan" not in BR.DIRECT
    gap, t = BR.strict_gap_per_pair("ref"), BR.forward_tol("ref")
    print(f"ref: strict gap per pair = {[f'{x:.3e}' for x in gap.tolist()]}, forward tol = {t:.3e}")
    assert bool((gap <= 2 * t).any())
