"""CPU tests of the fp8 token search: the C ABI declaration and the binding, every refusal of mm_dot_topk_fp8_fwd through the
raw binding (nothing is launched), the preconditions of the exact cases of tests/test_fp8_token_search_gpu.py from the
restatement alone, and TokenStore's token_search= / row_shard= host logic driven through numpy stand-ins."""
import os

import numpy as np
import pytest
import torch

from tests import dot_topk_reference as D
from tests import fp8_store_reference as F
from tests import fp8_token_search_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ C ABI and binding
def test_header_binding_and_exports_declare_the_entry():
    from matchmaker_amd import _lib, build, ops
    from tests import abi
    L = abi.assert_bound(("mm_dot_topk_fp8_workspace_bytes", "mm_dot_topk_fp8_fwd"))
    hdr = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    assert "dense_retrieval.py:391" in hdr[hdr.index("fp8 token search"):] and "faiss_indices.py:22-36" in hdr[hdr.index("fp8 token search"):]
    assert "dot_topk_fp8.hip" in build.SOURCES
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    assert callable(ops.dot_topk_fp8)
    from matchmaker_amd import torch_ops
    assert "dot_topk_fp8" not in open(torch_ops.__file__).read()           # like dot_topk: the loop reads status back


def test_every_refusal_is_reached_before_any_launch():
    from matchmaker_amd import _lib
    L = _lib.lib()
    p = 4096                                                               # any non-null aligned value: refused before it is used
    F16, BF16, F32 = _lib.MM_F16, _lib.MM_BF16, _lib.MM_F32
    assert L.mm_dot_topk_fp8_workspace_bytes(100, 4, 10) == L.mm_dot_topk_workspace_bytes(100, 4, 10) > 0
    assert L.mm_dot_topk_fp8_workspace_bytes(0, 4, 10) == 0
    big = 1 << 40

    def call(queries=p, codes=p, scales=p, n=100, nq=4, E=128, dt=F16, k=10, out_s=p, out_i=p, st=p, ws=p, wsb=big):
        return L.mm_dot_topk_fp8_fwd(queries, codes, scales, n, nq, E, dt, k, 1.0, out_s, out_i, st, ws, wsb, None)

    for E in (64, 100, 640, 1024, 136):
        assert call(E=E) == _lib.MM_EUNSUPPORTED
        assert b"pad the vectors" in L.mm_last_error()
    assert call(dt=F32) == _lib.MM_EUNSUPPORTED
    assert b"fp16 or bf16" in L.mm_last_error()
    assert call(k=4097) == _lib.MM_EUNSUPPORTED
    assert call(n=1 << 31) == _lib.MM_EUNSUPPORTED
    assert call(dt=7) == _lib.MM_EINVAL
    for kw in ({"queries": None}, {"codes": None}, {"scales": None}, {"out_s": None}, {"out_i": None}, {"st": None},
               {"n": 0}, {"n": -1}, {"nq": 0}, {"E": 0}, {"k": 0}):
        assert call(**kw) == _lib.MM_EINVAL, kw
    assert call(queries=p + 8) == _lib.MM_EINVAL and call(codes=p + 8) == _lib.MM_EINVAL and call(scales=p + 2) == _lib.MM_EINVAL
    assert b"aligned" in L.mm_last_error()
    need = L.mm_dot_topk_fp8_workspace_bytes(100, 4, 10)
    assert call(wsb=need - 1) == _lib.MM_EWORKSPACE and call(ws=None) == _lib.MM_EWORKSPACE
    for dt in (F16, BF16):                                                 # (a served dtype gets as far as the workspace check)
        assert call(dt=dt, wsb=0) == _lib.MM_EWORKSPACE


def test_operator_refuses_cpu_tensors():
    from matchmaker_amd import NativeError, ops
    q = torch.zeros(2, 128, dtype=torch.float16)
    codes = torch.zeros(5, 128, dtype=torch.uint8)
    scales = torch.ones(5)
    with pytest.raises(NativeError, match="CPU tensor"):             # (dtypes and shapes: checked on device tensors, GPU suite)
        ops.dot_topk_fp8(q, codes, scales, 3)


# ------------------------------------------------------------------------------------------ preconditions of the exact cases
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_scaled_cases_are_exact_fit_the_candidate_lists_and_hold_ties(case):
    _, dtype, nq, N, E, k, _ = case
    q, codes, scales = R.case_inputs(case)
    vals = F.deq_numpy(codes)
    assert np.abs(vals).max() <= 8 and np.array_equal(vals, np.round(vals)) and np.abs(q).max() <= 2
    assert set(np.log2(scales).tolist()) <= set(range(-3, 4))
    for dt in (torch.float16, torch.bfloat16):                             # the query's values are exact in both 16-bit types
        assert np.array_equal(torch.from_numpy(q).to(dt).float().numpy(), q)
    full = R.scores64(q, codes, scales)
    mags = R.magnitudes64(q, codes, scales)
    assert np.array_equal(full * 8, np.round(full * 8)) and mags.max() * 8 < 2 ** 24      # exact in fp32 in any order
    above, at = D.tie_stats(full, k)
    assert above.max() <= D.cap_of(N, k), (above.max(), D.cap_of(N, k))
    print(f"{case[0]}: at or above the k-th score <= {above.max()} of cap {D.cap_of(N, k)}; ties at the k-th score <= {at.max()}")
    if N > 64 and k < N:
        assert at.max() >= 2                                               # a tie group at the k-th rank is present


def test_raw_abi_case_gives_status_1_2_0():
    _, _, nq, N, E, k, _ = R.RAW_ABI
    assert N % 32 not in (0,) and N > D.SAMPLE
    q, codes, scales = R.case_inputs(R.RAW_ABI)
    full = R.scores64(q, codes, scales)
    assert np.array_equal(full * 8, np.round(full * 8))
    cap = D.cap_of(N, k)
    assert (D.sampled_survivors(full, k, 1e-3) < k).all()                  # status 1
    assert (D.sampled_survivors(full, k, 100.0) > cap).all()               # status 2
    n = D.sampled_survivors(full, k, 1.0)
    assert (n >= k).all() and (n <= cap).all(), n                          # status 0
    assert D.tie_stats(full, k)[0].max() <= cap


def test_the_existing_exact_stores_quantise_losslessly():
    for kind, want in (("ternary", 2.0 ** -7), ("quarter", None), ("nonpos", 2.0 ** -7)):
        q, c = D.inputs(kind, 3, 500, 128, 5)
        codes, scales = R.quantized(c)
        assert np.array_equal(F.dequantize_numpy(codes, scales), c.astype(np.float64)), kind
        if want is not None:
            assert set(scales[np.abs(c).max(axis=1) > 0].tolist()) == {want}
    q, c, rows, k = D.planted_sampled_1100()
    codes, scales = R.quantized(c)
    assert np.array_equal(F.dequantize_numpy(codes, scales), c.astype(np.float64))
    ref = R.dot_topk_fp8_exact(q, codes, scales, k)
    assert np.array_equal(ref[0], D.dot_topk_exact(q, c, k)[0]) and np.array_equal(ref[1], D.dot_topk_exact(q, c, k)[1])


def test_sharded_restatement_equals_the_unsharded_one_with_ties_across_a_boundary():
    rng = np.random.default_rng(3)
    full = rng.integers(0, 6, (4, 12100)).astype(np.float64)               # six values: every rank is inside a tie group
    for shard, k in ((4032, 100), (64, 7), (12100, 100), (20000, 100), (4032, 4096)):
        s, i = R.sharded_topk_of_scores(full, k, shard)
        ws, wi = D.topk_of_scores(full, k)
        assert np.array_equal(s, ws) and np.array_equal(i, wi), (shard, k)
    # the tie group at rank k straddles the boundary at row 4032
    _, wi = D.topk_of_scores(full, 3000)
    kth = full[0, wi[0, -1]]
    tied = np.nonzero(full[0] == kth)[0]
    assert tied.min() < 4032 < tied.max()
    s, i = R.sharded_topk_of_scores(full, 3000, 4032)
    assert np.array_equal(i, wi)


# ------------------------------------------------------------------------------------------ TokenStore through stand-ins
class _StandIns:
    """numpy stand-ins of the native searches and of the merge; they record how they were called"""

    def __init__(self):
        self.calls = []

    def quantize(self, x):
        return F.quantize_torch(x)

    def topk(self, q, matrix, k):
        self.calls.append(("topk", q.dtype, tuple(matrix.shape), k))
        s, i = D.dot_topk_exact(q.double().numpy(), matrix.double().numpy(), k)
        return torch.from_numpy(s).float(), torch.from_numpy(i)

    def topk_fp8(self, q, codes, scales, k):
        assert codes.dtype == torch.uint8 and scales.dtype == torch.float32 and scales.shape == (codes.shape[0],)
        self.calls.append(("topk_fp8", q.dtype, tuple(codes.shape), k))
        s, i = R.dot_topk_fp8_exact(q.double().numpy(), codes.numpy(), scales.numpy(), k)
        return torch.from_numpy(s).float(), torch.from_numpy(i)

    def merge(self, scores, ids, k):
        self.calls.append(("merge", tuple(scores.shape), k))
        s, i = D.topk_merge_exact(scores.numpy(), ids.numpy(), k)
        return torch.from_numpy(s).float(), torch.from_numpy(i)

    def fns(self):
        return {"topk_fn": self.topk, "topk_fp8_fn": self.topk_fp8, "merge_fn": self.merge, "quantize_fn": self.quantize}


def _store(fn, T=300, E=16, dtype=torch.float16, seed=2):
    """a store of T rows in documents of 5: values multiples of 1/8 up to 2 (lossless in fp8), many equal rows -> ties"""
    from matchmaker_amd.token_store import TokenStore
    rng = np.random.default_rng(seed)
    tokens = torch.from_numpy(rng.integers(-2, 3, (T, E)) / 8.0).to(dtype)
    tokens[tokens.abs().sum(-1) == 0, 0] = 0.125
    end = np.minimum(np.arange(5, T + 5, 5), T)
    begin = np.arange(0, T, 5)
    ids = [f"d{i}" for i in range(len(begin))]
    return TokenStore(tokens, ids, begin, end, **fn.fns()), tokens


def _queries(nq=2, Q=3, E=16, seed=9):
    q = torch.from_numpy(np.random.default_rng(seed).integers(-2, 3, (nq, Q, E)).astype(np.float32))
    q[0, 1] = 0                                                            # a dead query token
    return q


@pytest.mark.parametrize("src, want", [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16),
                                       (torch.float32, torch.float16)])
def test_token_search_fp8_calls_the_injected_search_with_codes_scales_and_the_source_dtype(src, want, tmp_path):
    from matchmaker_amd.token_store import TokenStore
    fn = _StandIns()
    st, tokens = _store(fn, dtype=src)
    f8 = st.quantize_fp8()                                                 # fp8-ONLY: no 16-bit rows
    assert torch.equal(F.dequantize_torch(f8.codes, f8.scales, src), tokens)
    q = _queries()
    fn.calls.clear()
    hits = f8.token_hits(q, 4, token_search="fp8")
    assert fn.calls == [("topk_fp8", want, (300, 16), 4)]
    ref = R.dot_topk_fp8_exact(q.reshape(6, 16).numpy(), f8.codes.numpy(), f8.scales.numpy(), 4)[1].reshape(2, 3, 4)
    ref[0, 1] = -1                                                         # the dead token
    assert hits.shape == (2, 12) and np.array_equal(hits.numpy().reshape(2, 3, 4), ref)
    # the function is carried through save_fp8 / load_fp8, from_reference_parts and quantize_fp8
    f8.save_fp8(str(tmp_path / "fp8"))
    back = TokenStore.load_fp8(str(tmp_path / "fp8"), "cpu", **fn.fns())
    fn.calls.clear()
    assert torch.equal(back.token_hits(q, 4, token_search="fp8"), hits) and fn.calls[0][:2] == ("topk_fp8", want)
    parts = TokenStore.from_reference_parts([tokens.numpy() if src != torch.bfloat16 else tokens.float().numpy()],
                                            {s: (0, int(b), int(e)) for s, b, e in zip(st.seq_ids, st._begin, st._end)},
                                            st.seq_ids, "cpu", fp8=True, **fn.fns())
    fn.calls.clear()
    assert torch.equal(parts.token_hits(q, 4, token_search="fp8"), hits) and fn.calls[0][0] == "topk_fp8"


def test_default_still_refuses_and_the_misuses_raise():
    from matchmaker_amd import NativeError, _lib
    fn = _StandIns()
    st, _ = _store(fn)
    f8 = st.quantize_fp8()
    q = _queries()
    with pytest.raises(NativeError, match="an fp8 store holds no 16-bit rows to search — pass index=.*keep_tokens=True") as ei:
        f8.token_hits(q, 4)
    assert ei.value.code == _lib.MM_EUNSUPPORTED and 'token_search="fp8"' in str(ei.value)
    with pytest.raises(NativeError, match="keep_tokens=True"):
        f8.search_device(q, 3, 4)
    with pytest.raises(NativeError, match="needs an fp8 store"):
        st.token_hits(q, 4, token_search="fp8")
    with pytest.raises(NativeError, match="token_search='fp16'"):
        f8.token_hits(q, 4, token_search="fp16")

    class _Index:
        def search_device(self, qs, k):
            return None, torch.arange(k).repeat(qs.shape[0], 1)

    with pytest.raises(NativeError, match="two searches"):
        f8.token_hits(q, 4, index=_Index(), token_search="fp8")
    with pytest.raises(NativeError, match="not with index="):
        f8.token_hits(q, 4, index=_Index(), row_shard=64)
    for bad in (0, -64, 100, 63, 64.5):
        with pytest.raises(NativeError, match="positive multiple of 64"):
            f8.token_hits(q, 4, token_search="fp8", row_shard=bad)
    # a kept-rows store searches its 16-bit rows by default and its codes on request
    kept = st.quantize_fp8(keep_tokens=True)
    fn.calls.clear()
    a = kept.token_hits(q, 4)
    b = kept.token_hits(q, 4, token_search="fp8")
    assert [c[0] for c in fn.calls] == ["topk", "topk_fp8"] and torch.equal(a, b)      # lossless store: the same hits


@pytest.mark.parametrize("T, shard, k", [(12100, 4032, 100), (300, 64, 7), (300, 320, 7), (320, 320, 7), (200, 128, 150)])
def test_row_shard_equals_the_unsharded_restatement_on_both_paths(T, shard, k):
    fn = _StandIns()
    st, tokens = _store(fn, T=T, seed=T)
    f8 = st.quantize_fp8()
    q = _queries(nq=1, Q=2)
    q[0, 1] = torch.from_numpy(np.random.default_rng(1).integers(-2, 3, 16).astype(np.float32))
    full = q.reshape(2, 16).double().numpy() @ tokens.double().numpy().T
    want = D.topk_of_scores(full, k)[1]
    at = D.tie_stats(full, k)[1]
    assert at.max() >= 2                                                   # ties at the k-th rank
    assert np.array_equal(R.sharded_topk_of_scores(full, k, shard)[1], want)
    for store, kw, name in ((st, {}, "topk"), (f8, {"token_search": "fp8"}, "topk_fp8")):
        fn.calls.clear()
        hits = store.token_hits(q, k, row_shard=shard, **kw)
        assert np.array_equal(hits.numpy().reshape(2, k), want), name
        n_shards = 1 if shard >= T else -(-T // shard)
        searches = [c for c in fn.calls if c[0] == name]
        assert len(searches) == n_shards and [c[0] for c in fn.calls].count("merge") == n_shards - 1
        assert all(c[1] == (2, 2 * k) for c in fn.calls if c[0] == "merge")
        assert sum(c[2][0] for c in searches) == T


def test_search_device_and_search_pass_the_options_to_token_hits():
    fn = _StandIns()
    st, _ = _store(fn)
    f8 = st.quantize_fp8()
    seen = []
    f8.token_hits = lambda qv, k, **kw: seen.append(kw) or torch.zeros(qv.shape[0], qv.shape[1] * k, dtype=torch.int64)
    f8.rank_hits = lambda qv, hits, top_n, **kw: (torch.zeros(qv.shape[0], top_n), torch.zeros(qv.shape[0], top_n, dtype=torch.int64))
    q = _queries()
    f8.search_device(q, 3, 4, token_search="fp8", row_shard=128)
    f8.search(q, 3, 4, token_search="fp8", row_shard=64)
    f8.search_device(q, 3, 4)
    assert [(kw["token_search"], kw["row_shard"]) for kw in seen] == [("fp8", 128), ("fp8", 64), (None, None)]
