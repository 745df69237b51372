"""Exact-tie and large-k tests of mm_dot_topk_fwd / mm_topk_merge against tests/dot_topk_reference.py.

Every store here has inner products that are exact in fp32 in any summation order (and values exact in float16 and
bfloat16), so every assertion is EQUALITY of scores and rows with the float64 restatement: "ties: lower row first" for
mm_dot_topk_fwd, "input order on ties" for mm_topk_merge.  The tie-count preconditions of the cases (documents at or above
the k-th score against the candidate capacity, rows above / below the 1,024-entry selection limit) are asserted from the
reference alone in tests/test_dot_topk_reference_cpu.py."""
import numpy as np
import pytest
import torch

from tests import dot_topk_reference as R
from tests import util

pytestmark = pytest.mark.gpu

TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def _search(q, c, k, dtype="float16"):
    """ops.dot_topk on float32 numpy holding 16-bit-exact values -> numpy (scores, rows)"""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    dt = TORCH_DT[dtype]
    s, i = ops.dot_topk(torch.from_numpy(q).to(dev).to(dt), torch.from_numpy(c).to(dev).to(dt), k)
    torch.cuda.synchronize(dev)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and s.shape == i.shape == (q.shape[0], k)
    return s.cpu().numpy(), i.cpu().numpy()


def _equal(got, ref, label=""):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=f"{label}: scores")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{label}: rows")


def _run_case(case):
    name, _, dtype, _, _, _, k, _ = case
    q, c = R.case_inputs(case)
    ref = R.dot_topk_exact(q, c, k)
    _equal(_search(q, c, k, dtype), ref, name)
    return q, c, ref


@pytest.mark.parametrize("case", R.SWEEP, ids=[c[0] for c in R.SWEEP])
def test_instantiations_bit_equal_with_ties(case):
    _run_case(case)


@pytest.mark.parametrize("case", R.LARGE_K, ids=[c[0] for c in R.LARGE_K])
def test_k_above_1024_takes_the_full_sort(case):
    _, _, _, nq, N, _, k, _ = case
    _, _, (ref_s, ref_i) = _run_case(case)
    if N < k:        # the reference (and so the device) pads exactly the tail
        assert (ref_i[:, :N] >= 0).all() and (ref_i[:, N:] == -1).all() and np.isneginf(ref_s[:, N:]).all()


def test_k_above_4096_is_refused():
    from matchmaker_amd import _lib, ops
    dev = util.require_gpu()
    q, c = R.inputs("ternary", 2, 6000, 128, 35)
    with pytest.raises(_lib.NativeError) as e:
        ops.dot_topk(torch.from_numpy(q).to(dev).half(), torch.from_numpy(c).to(dev).half(), R.K_MAX + 1)
    assert e.value.code == _lib.MM_EUNSUPPORTED
    # the same call at the limit is served
    _equal(_search(q, c, R.K_MAX), R.dot_topk_exact(q, c, R.K_MAX), "k = 4096")


def test_rows_above_and_below_the_selection_limit_in_one_call():
    q, c = R.mixed_ties_inputs()
    k = R.MIXED_TIES[6]
    _equal(_search(q, c, k), R.dot_topk_exact(q, c, k), "mixed ties")


def test_planted_group_of_1500_best_returns_its_lowest_1000_rows():
    q, c, rows, k = R.planted_1500()
    s, i = _search(q, c, k)
    np.testing.assert_array_equal(i[0], rows[:k])
    np.testing.assert_array_equal(s[0], np.full(k, c.shape[1], np.float32))
    _equal((s, i), R.dot_topk_exact(q, c, k), "planted 1500")


def test_tie_group_across_the_sampled_threshold_and_the_selection():
    q, c, rows, k = R.planted_sampled_1100()
    s, i = _search(q, c, k)
    np.testing.assert_array_equal(i[0], rows[:k])
    _equal((s, i), R.dot_topk_exact(q, c, k), "planted sampled 1100")


def test_all_zero_query_returns_the_first_rows():
    q, c = R.inputs("ternary", 3, 3000, 128, 76)
    q[1] = 0
    s, i = _search(q, c, 100)
    np.testing.assert_array_equal(i[1], np.arange(100))
    np.testing.assert_array_equal(s[1], np.zeros(100, np.float32))
    _equal((s, i), R.dot_topk_exact(q, c, 100), "all-zero query")


def test_more_ties_than_candidate_slots_raise_the_documented_error():
    from matchmaker_amd import _lib, ops
    dev = util.require_gpu()
    q, c, _, k = R.planted_5000()
    with pytest.raises(_lib.NativeError, match="without an exact top-1000"):
        ops.dot_topk(torch.from_numpy(q).to(dev).half(), torch.from_numpy(c).to(dev).half(), k)
    q, c = R.inputs("ternary", 2, 20000, 128, 77)
    q[0] = 0
    with pytest.raises(_lib.NativeError, match="without an exact top-100"):
        ops.dot_topk(torch.from_numpy(q).to(dev).half(), torch.from_numpy(c).to(dev).half(), 100)
    # the device is in order afterwards: the row that can be served is served
    _equal(_search(q[1:], c, 100), R.dot_topk_exact(q[1:], c, 100), "after the refusal")


@pytest.mark.parametrize("case", R.NEGATIVE, ids=[c[0] for c in R.NEGATIVE])
def test_all_negative_rows_hold_real_documents_only(case):
    _, _, (ref_s, ref_i) = _run_case(case)
    assert (ref_s < 0).all() and (ref_i >= 0).all()


def test_more_than_32_query_groups():
    _run_case(R.MANY_GROUPS)


@pytest.mark.parametrize("k", [10, 100])
def test_shard_smaller_than_k_pads_exactly_the_tail(k):
    for N in (1, k - 1, k):
        q, c = R.inputs("ternary", 3, N, 128, 78 + N)
        s, i = _search(q, c, k)
        _equal((s, i), R.dot_topk_exact(q, c, k), f"N = {N}")
        assert (i[:, :N] >= 0).all() and (i[:, N:] == -1).all() and np.isneginf(s[:, N:]).all()


# ---- the C ABI: status / m_scale, buffers, workspace ------------------------------------------------------------------

GUARD = 256   # bytes (a multiple of every alignment the call needs)


def _guarded(n_bytes, fill, dev):
    """a byte tensor [GUARD | n_bytes | GUARD] filled with `fill` -> (tensor, interior pointer)"""
    t = torch.full((n_bytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return t, t.data_ptr() + GUARD


def _guards_intact(t, fill):
    return bool((t[:GUARD] == fill).all()) and bool((t[-GUARD:] == fill).all())


def test_raw_abi_status_follows_m_scale_and_nothing_leaves_its_buffers():
    from matchmaker_amd import _lib, ops
    dev = util.require_gpu()
    _, _, dtype, nq, N, E, k, _ = R.RAW_ABI
    q, c = R.case_inputs(R.RAW_ABI)
    ref_s, ref_i = R.dot_topk_exact(q, c, k)
    qd = torch.from_numpy(q).to(dev).to(TORCH_DT[dtype])
    cd = torch.from_numpy(c).to(dev).to(TORCH_DT[dtype])
    L = _lib.lib()
    wsb = L.mm_dot_topk_workspace_bytes(N, nq, k)
    assert wsb > 0
    FILL = 0xA5
    bufs = {name: _guarded(n, FILL, dev) for name, n in
            (("scores", nq * k * 4), ("idx", nq * k * 8), ("status", nq * 4), ("ws", wsb))}

    def call(m_scale, ws_bytes=wsb):
        for t, _ in bufs.values():
            t.fill_(FILL)
        with torch.cuda.device(dev):
            rc = L.mm_dot_topk_fwd(qd.data_ptr(), cd.data_ptr(), N, nq, E, ops._DT[qd.dtype], k, m_scale, bufs["scores"][1],
                                   bufs["idx"][1], bufs["status"][1], bufs["ws"][1], ws_bytes, ops._stream(dev))
        torch.cuda.synchronize(dev)
        inner = lambda name, dt: bufs[name][0][GUARD:-GUARD].view(dt).cpu().numpy()   # noqa: E731
        return rc, inner("scores", torch.float32).reshape(nq, k), inner("idx", torch.int64).reshape(nq, k), \
            inner("status", torch.int32)

    for m_scale, want in ((1e-3, 1), (100.0, 2), (1.0, 0)):
        rc, s, i, st = call(m_scale)
        assert rc == _lib.MM_OK, L.mm_last_error()
        np.testing.assert_array_equal(st, np.full(nq, want, np.int32), err_msg=f"m_scale = {m_scale}")
        for name, (t, _) in bufs.items():
            assert _guards_intact(t, FILL), f"m_scale = {m_scale}: bytes around `{name}` were written"
        if want == 0:
            np.testing.assert_array_equal(s, ref_s)
            np.testing.assert_array_equal(i, ref_i)
    # one byte less than mm_dot_topk_workspace_bytes: refused, nothing written
    rc, s, i, st = call(1.0, wsb - 1)
    assert rc == _lib.MM_EWORKSPACE
    for t, _ in bufs.values():
        assert bool((t == FILL).all())


# ---- determinism -------------------------------------------------------------------------------------------------------

def test_two_calls_are_bit_equal_and_a_row_does_not_depend_on_its_batch():
    q, c = R.inputs("ternary", 257, 20000, 256, 79)
    a = _search(q, c, 100)
    b = _search(q, c, 100)
    _equal(b, a, "second call")
    one = _search(q[:1], c, 100)                    # one query tile alone against two tiles with a partial group
    _equal(one, (a[0][:1], a[1][:1]), "nq = 1 against row 0 of nq = 257")
    _equal(a, R.dot_topk_exact(q, c, 100), "reference")


# ---- mm_topk_merge -----------------------------------------------------------------------------------------------------

def _merge(s, ids, k):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    ms, mi = ops.topk_merge(torch.from_numpy(s).to(dev), torch.from_numpy(ids).to(dev), k)
    torch.cuda.synchronize(dev)
    assert ms.dtype == torch.float32 and mi.dtype == torch.int64 and ms.shape == mi.shape == (s.shape[0], k)
    return ms.cpu().numpy(), mi.cpu().numpy()


@pytest.mark.parametrize("n_in", [1, 2, 1000, R.MERGE_MAX])
def test_topk_merge_bit_equal_with_ties_padding_and_wide_ids(n_in):
    s, ids = R.merge_inputs(n_in)
    for k in sorted({1, n_in, n_in + 5}):
        _equal(_merge(s, ids, k), R.topk_merge_exact(s, ids, k), f"n_in = {n_in}, k = {k}")


def test_topk_merge_refuses_more_than_16384_inputs():
    from matchmaker_amd import _lib
    s = np.zeros((3, R.MERGE_MAX + 1), np.float32)
    ids = np.tile(np.arange(R.MERGE_MAX + 1, dtype=np.int64), (3, 1))
    with pytest.raises(_lib.NativeError) as e:
        _merge(s, ids, 10)
    assert e.value.code == _lib.MM_EUNSUPPORTED


def test_merge_of_shard_results_equals_the_search_of_the_whole():
    q, c = R.shard_inputs()
    k = 100
    parts_s, parts_i, lo = [], [], 0
    for n in R.SHARDS:
        s, i = _search(q, c[lo: lo + n], k)
        _equal((s, i), R.dot_topk_exact(q, c[lo: lo + n], k), f"shard at {lo}")
        parts_s.append(s)
        parts_i.append(np.where(i >= 0, i + lo, -1))
        lo += n
    assert (parts_i[-1][:, R.SHARDS[-1]:] == -1).all()            # the last shard is smaller than k: padded
    merged = _merge(np.concatenate(parts_s, axis=1), np.concatenate(parts_i, axis=1), k)
    whole = _search(q, c, k)
    _equal(merged, whole, "merge of the shards against the whole corpus")
    _equal(whole, R.dot_topk_exact(q, c, k), "whole corpus")
