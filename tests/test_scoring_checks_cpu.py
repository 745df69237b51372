"""CPU test of the argument checks the scoring operators share (matchmaker_amd.ops: MaxSim and its ragged, fp8, all-pairs and
backward forms, kernel pooling, PACRR, CO-PACRR, DRMM, MatchPyramid): every operator raises every shared check with the text
and the NativeError code it had when each wrapper spelled the check out itself.  Fake tensors "on" the device pass the
CPU-tensor refusal, which comes first, and every check below runs before anything touches a device."""
import pytest
import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _t(*shape, dtype=F16):
    return torch.empty(*shape, dtype=dtype, device="cuda")


def _qd(dtype=F16, nq=3, B=3, E=128, E2=None, ddtype=None):
    """q [nq, 5, E], d [B, 7, E2 or E]"""
    return _t(nq, 5, E, dtype=dtype), _t(B, 7, E if E2 is None else E2, dtype=dtype if ddtype is None else ddtype)


def _rbf():
    return tuple(_t(11, dtype=F32) for _ in range(4))


VIEWS = [2, 4, 6, 7]


# operator -> how it is called with a (q, d) pair (and pairs_per_query where it takes one); everything else valid
def _call_qd(ops, op, q, d, ppq=1):
    B, Q = d.shape[0], q.shape[1]
    return {
        "maxsim": lambda: ops.maxsim(q, d, pairs_per_query=ppq),
        "maxsim_bwd": lambda: ops.maxsim_bwd(q, d, None, None, _t(B, dtype=F32)),
        "maxsim_inbatch": lambda: ops.maxsim_inbatch(q, None, d, None),
        "maxsim_inbatch_bwd": lambda: ops.maxsim_inbatch_bwd(q, None, d, None, _t(q.shape[0], B, dtype=F32)),
        "kernel_pool": lambda: ops.kernel_pool(q, d, None, None, *_rbf(), pairs_per_query=ppq),
        "kernel_pool_bwd": lambda: ops.kernel_pool_bwd(q, d, None, None, *_rbf(), _t(B, dtype=F32)),
        "pacrr_kmax": lambda: ops.pacrr_kmax(q, d, [], [], 2, pairs_per_query=ppq),
        "pacrr_kmax_bwd": lambda: ops.pacrr_kmax_bwd(q, d, [], _t(B, Q, 2, dtype=torch.int32), _t(B, Q, 2, dtype=F32), 2, ppq),
        "co_pacrr_kmax": lambda: ops.co_pacrr_kmax(q, d, [], [], 2, VIEWS, pairs_per_query=ppq),
        "co_pacrr_kmax_bwd": lambda: ops.co_pacrr_kmax_bwd(q, d, [], _t(B, Q, 1, 8, dtype=torch.int32),
                                                           _t(B, Q, 16, dtype=F32), 2, VIEWS, ppq),
        "drmm_hist": lambda: ops.drmm_hist(q, d, pairs_per_query=ppq),
        "drmm_score": lambda: ops.drmm_score(q, d, _t(q.shape[0], Q, dtype=F32), _t(10, 10, dtype=F32), _t(10, dtype=F32),
                                             _t(10, dtype=F32), _t(1, dtype=F32), pairs_per_query=ppq),
        "matchpyramid_features": lambda: ops.matchpyramid_features(q, d, [], [], [], pairs_per_query=ppq),
    }[op]()


SAME_DTYPE = ("maxsim", "maxsim_bwd", "maxsim_inbatch", "maxsim_inbatch_bwd")                 # 16-bit or fp32 vectors
FP32_ONLY = ("kernel_pool", "kernel_pool_bwd", "pacrr_kmax", "pacrr_kmax_bwd", "co_pacrr_kmax", "co_pacrr_kmax_bwd", "drmm_hist",
             "drmm_score", "matchpyramid_features")
PAIR_PER_ROW = ("maxsim_bwd", "kernel_pool_bwd")                                            # the backwards' layout
PER_QUERY = ("maxsim", "kernel_pool", "pacrr_kmax", "pacrr_kmax_bwd", "co_pacrr_kmax", "co_pacrr_kmax_bwd", "drmm_hist",
             "drmm_score", "matchpyramid_features")


def _raises(fn, text, code=None):
    from matchmaker_amd import NativeError
    with pytest.raises(NativeError) as err:
        fn()
    assert str(err.value) == text, (str(err.value), text)
    assert err.value.code == code, text


@pytest.mark.parametrize("op", SAME_DTYPE + FP32_ONLY)
def test_every_shared_check_of_the_embedding_pair_keeps_its_text(op):
    from matchmaker_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    dtype = F16 if op in SAME_DTYPE else F32
    with FakeTensorMode():
        if op in SAME_DTYPE:
            q, d = _qd(F16, ddtype=BF16)
            _raises(lambda: _call_qd(ops, op, q, d), "q/d dtype mismatch: torch.float16 vs torch.bfloat16")
        q, d = _qd(dtype, E=128, E2=64)
        if op in PAIR_PER_ROW:
            _raises(lambda: _call_qd(ops, op, q, d), f"{op} needs the pair-per-row layout: q (3, 5, 128) vs d (3, 7, 64)")
            q, d = _qd(dtype, nq=2, B=3)
            _raises(lambda: _call_qd(ops, op, q, d), f"{op} needs the pair-per-row layout: q (2, 5, 128) vs d (3, 7, 128)")
        else:
            _raises(lambda: _call_qd(ops, op, q, d), "embedding dims differ: 128 vs 64")
        if op in PER_QUERY:
            q, d = _qd(dtype, nq=3, B=2)
            _raises(lambda: _call_qd(ops, op, q, d), "q has 3 rows but 2 pairs / 1 per query")
            q, d = _qd(dtype, nq=2, B=7)
            _raises(lambda: _call_qd(ops, op, q, d, ppq=3), "q has 2 rows but 7 pairs / 3 per query")
            _raises(lambda: _call_qd(ops, op, q, d, ppq=0), "q has 2 rows but 7 pairs / 0 per query")


def test_the_backwards_share_the_grad_out_and_gradient_dtype_checks():
    from matchmaker_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q, d = _qd(F16)
        _raises(lambda: ops.maxsim_bwd(q, d, None, None, _t(4, dtype=F32)), "grad_out has 4 elements for 3 pairs")
        _raises(lambda: ops.maxsim_bwd(q, d, None, None, _t(3, dtype=F32), grad_dtype=BF16),
                "maxsim_bwd: gradients are float32 or torch.float16, not torch.bfloat16")
        q, d = _qd(BF16, nq=2, B=3)
        _raises(lambda: ops.maxsim_inbatch_bwd(q, None, d, None, _t(2, 2, dtype=F32)), "grad_out has 4 elements for 2 x 3 pairs")
        _raises(lambda: ops.maxsim_inbatch_bwd(q, None, d, None, _t(2, 3, dtype=F32), grad_dtype=F16),
                "maxsim_inbatch_bwd: gradients are float32 or torch.bfloat16, not torch.float16")
        q, d = _qd(F32)
        _raises(lambda: ops.kernel_pool_bwd(q, d, None, None, *_rbf(), _t(2, 2, dtype=F32)), "grad_out has 4 elements for 3 pairs")


def _ragged(ops, op, q, doc_begin, doc_end, E_store=128, ppq=1):
    if op == "maxsim_ragged":
        return ops.maxsim_ragged(q, _t(20, E_store), doc_begin, doc_end, pairs_per_query=ppq)
    return ops.maxsim_ragged_fp8(q, _t(20, E_store, dtype=torch.uint8), _t(20, dtype=F32), doc_begin, doc_end, pairs_per_query=ppq)


def test_the_two_ragged_operators_give_one_text_for_one_mistake():
    from matchmaker_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    i64 = torch.int64
    with FakeTensorMode():
        for op in ("maxsim_ragged", "maxsim_ragged_fp8"):
            q = _t(2, 5, 128)
            _raises(lambda: _ragged(ops, op, q, _t(3, dtype=i64), _t(2, dtype=i64)), "doc_begin / doc_end must have one entry per pair")
            _raises(lambda: _ragged(ops, op, q, _t(3, dtype=i64), _t(3, dtype=i64)), "q has 2 rows but 3 pairs / 1 per query")
            _raises(lambda: _ragged(ops, op, q, _t(3, dtype=i64), _t(3, dtype=i64), ppq=0), "q has 2 rows but 3 pairs / 0 per query")
            _raises(lambda: _ragged(ops, op, q, _t(2, dtype=i64), _t(2, dtype=i64), E_store=64), "embedding dims differ: 128 vs 64")
