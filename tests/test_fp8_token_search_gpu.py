"""GPU tests of the fp8 token search (mm_dot_topk_fp8_fwd / ops.dot_topk_fp8) against
tests/fp8_token_search_reference.py, and of TokenStore's token_search="fp8" / row_shard= end to end.

On the exact stores every score is exact in fp32 in any summation order, so the assertions are EQUALITY of scores and rows with
the float64 restatement, ties included ("lower row first").  On random data the per-score bound is
(E + 2) 2^-24 scales[t] sum_k |q_k| |deq_tk| (E fp32 additions, exact products, exact scale).  The preconditions of the exact
cases are asserted from the reference alone in tests/test_fp8_token_search_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import colbert_search_reference as CR
from tests import dot_topk_reference as D
from tests import fp8_store_reference as F
from tests import fp8_token_search_reference as R
from tests import util

pytestmark = pytest.mark.gpu

TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def _search(q, codes, scales, k, dtype="float16"):
    """ops.dot_topk_fp8 on numpy inputs (q float32 holding 16-bit-exact values) -> numpy (scores, rows)"""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    s, i = ops.dot_topk_fp8(torch.from_numpy(q).to(dev).to(TORCH_DT[dtype]), torch.from_numpy(codes).to(dev),
                            torch.from_numpy(scales).to(dev), k)
    torch.cuda.synchronize(dev)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and s.shape == i.shape == (q.shape[0], k)
    return s.cpu().numpy(), i.cpu().numpy()


def _equal(got, ref, label=""):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=f"{label}: scores")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{label}: rows")


def _quantize_on_device(c, dtype="float16"):
    """ops.fp8_quantize_rows of a float32 numpy corpus holding 16-bit-exact values -> numpy (codes, scales)"""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    codes, scales = ops.fp8_quantize_rows(torch.from_numpy(c).to(dev).to(TORCH_DT[dtype]))
    return codes.cpu().numpy(), scales.cpu().numpy()


# ---- bit equality with ties on the scaled store -----------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_scaled_store_bit_equal_with_ties(case):
    name, dtype, _, N, _, k, _ = case
    q, codes, scales = R.case_inputs(case)
    ref = R.dot_topk_fp8_exact(q, codes, scales, k)
    got = _search(q, codes, scales, k, dtype)
    _equal(got, ref, name)
    if N < k:
        assert (got[1][:, :N] >= 0).all() and (got[1][:, N:] == -1).all() and np.isneginf(got[0][:, N:]).all()


# ---- the existing exact stores, quantised -----------------------------------------------------------------------------

def _quantized_equals_the_16_bit_reference(q, c, k, dtype, label):
    codes, scales = _quantize_on_device(c, dtype)
    assert np.array_equal(F.dequantize_numpy(codes, scales), c.astype(np.float64)), f"{label}: the store is not lossless"
    got = _search(q, codes, scales, k, dtype)
    _equal(got, D.dot_topk_exact(q, c, k), label)
    return got


@pytest.mark.parametrize("case", D.NEGATIVE, ids=[c[0] for c in D.NEGATIVE])
def test_all_negative_rows_hold_real_rows_only(case):
    name, _, dtype, _, _, _, k, _ = case
    q, c = D.case_inputs(case)
    s, i = _quantized_equals_the_16_bit_reference(q, c, k, dtype, name)
    assert (s < 0).all() and (i >= 0).all()


def test_tie_groups_across_the_sampled_threshold_and_the_selection():
    q, c, rows, k = D.planted_sampled_1100()
    s, i = _quantized_equals_the_16_bit_reference(q, c, k, "float16", "planted sampled 1100")
    np.testing.assert_array_equal(i[0], rows[:k])
    q, c, rows, k = D.planted_1500()
    s, i = _quantized_equals_the_16_bit_reference(q, c, k, "bfloat16", "planted 1500")
    np.testing.assert_array_equal(i[0], rows[:k])
    np.testing.assert_array_equal(s[0], np.full(k, c.shape[1], np.float32))


def test_all_zero_query_returns_the_first_rows():
    q, c = D.inputs("ternary", 3, 3000, 128, 76)
    q[1] = 0
    s, i = _quantized_equals_the_16_bit_reference(q, c, 100, "float16", "all-zero query")
    np.testing.assert_array_equal(i[1], np.arange(100))
    np.testing.assert_array_equal(s[1], np.zeros(100, np.float32))


# ---- random data and threshold re-runs: the bound ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype, E, N", R.RANDOM, ids=[f"{d}-e{E}-n{N}" for d, E, N in R.RANDOM])
def test_random_rows_within_the_score_bound(dtype, E, N):
    q, codes, scales = R.random_inputs(dtype, E, N)
    full, bound = R.scores64(q, codes, scales), R.score_bound(q, codes, scales)
    for k in (10, 128):
        s, i = _search(q, codes, scales, k, dtype)
        worst = R.check_within_bound(full, bound, k, s, i)
        print(f"{dtype} E {E} N {N} k {k}: worst |error| / bound = {worst:.4f}")


def test_skewed_scores_need_threshold_reruns():
    """The store of test_dot_topk_skewed_scores_need_threshold_reruns, quantised: the strided sample misses the dense head, the
    sampled threshold lets too few / too many candidates through and the status-driven re-runs still deliver the top-k."""
    g = torch.Generator().manual_seed(5)
    N, E, k, nq = 60000, 128, 1000, 4
    c = (torch.randn(N, E, generator=g) * 0.05).half()
    q = torch.randn(nq, E, generator=g).half()
    rows = torch.arange(1, 6001, 2)
    c[rows] = (q[1].float() * (1.0 + 0.001 * torch.arange(rows.numel())[:, None])).half() * 0.1
    codes, scales = _quantize_on_device(c.float().numpy())
    qn = q.float().numpy()
    s, i = _search(qn, codes, scales, k)
    worst = R.check_within_bound(R.scores64(qn, codes, scales), R.score_bound(qn, codes, scales), k, s, i)
    print(f"skewed store: worst |error| / bound = {worst:.4f}")


# ---- the C ABI: status / m_scale, buffers, workspace, interior views ---------------------------------------------------

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
    _, _, nq, N, E, k, _ = R.RAW_ABI                                       # N % 32 = 19: a partial last block
    q, codes, scales = R.case_inputs(R.RAW_ABI)
    ref_s, ref_i = R.dot_topk_fp8_exact(q, codes, scales, k)
    qd = torch.from_numpy(q).to(dev).half()
    # codes and scales are interior views: the rows around them hold NaN codes (0x7f) and NaN scales — a load past either end
    # of the store would put a NaN into a score
    PAD = 64
    cbig = torch.full((N + 2 * PAD, E), 0x7f, dtype=torch.uint8, device=dev)
    sbig = torch.full((N + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)
    cbig[PAD: PAD + N] = torch.from_numpy(codes).to(dev)
    sbig[PAD: PAD + N] = torch.from_numpy(scales).to(dev)
    cd, sd = cbig[PAD: PAD + N], sbig[PAD: PAD + N]
    assert cd.data_ptr() % 16 == 0 and sd.data_ptr() % 4 == 0
    L = _lib.lib()
    wsb = L.mm_dot_topk_fp8_workspace_bytes(N, nq, k)
    assert wsb > 0
    FILL = 0xA5
    bufs = {name: _guarded(n, FILL, dev) for name, n in
            (("scores", nq * k * 4), ("idx", nq * k * 8), ("status", nq * 4), ("ws", wsb))}

    def call(m_scale, ws_bytes=wsb):
        for t, _ in bufs.values():
            t.fill_(FILL)
        with torch.cuda.device(dev):
            rc = L.mm_dot_topk_fp8_fwd(qd.data_ptr(), cd.data_ptr(), sd.data_ptr(), N, nq, E, ops._DT[qd.dtype], k, m_scale,
                                       bufs["scores"][1], bufs["idx"][1], bufs["status"][1], bufs["ws"][1], ws_bytes,
                                       ops._stream(dev))
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
    # one byte less than mm_dot_topk_fp8_workspace_bytes: refused, nothing written
    rc, s, i, st = call(1.0, wsb - 1)
    assert rc == _lib.MM_EWORKSPACE
    for t, _ in bufs.values():
        assert bool((t == FILL).all())
    # the store around the views was only read
    assert bool((cbig[:PAD] == 0x7f).all()) and bool((cbig[PAD + N:] == 0x7f).all()) and bool(sbig[:PAD].isnan().all())


def test_small_interior_view_reads_nothing_outside_itself():
    """N = 45 (two blocks, the second partial) inside NaN rows, through the operator: every row is a candidate, so a row
    read from outside the view would show up in the result."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, codes, scales = R.scaled_store(70, 45, 256, 162)
    cbig = torch.full((45 + 128, 256), 0x7f, dtype=torch.uint8, device=dev)
    sbig = torch.full((45 + 128,), float("nan"), dtype=torch.float32, device=dev)
    cbig[64: 64 + 45] = torch.from_numpy(codes).to(dev)
    sbig[64: 64 + 45] = torch.from_numpy(scales).to(dev)
    s, i = ops.dot_topk_fp8(torch.from_numpy(q).to(dev).to(torch.bfloat16), cbig[64: 64 + 45], sbig[64: 64 + 45], 45)
    _equal((s.cpu().numpy(), i.cpu().numpy()), R.dot_topk_fp8_exact(q, codes, scales, 45), "interior view")


def test_empty_inputs_behave_as_in_dot_topk():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q = torch.ones(3, 128, dtype=torch.float16, device=dev)
    codes = torch.zeros(0, 128, dtype=torch.uint8, device=dev)
    scales = torch.zeros(0, dtype=torch.float32, device=dev)
    s, i = ops.dot_topk_fp8(q, codes, scales, 5)
    assert s.shape == i.shape == (3, 5) and bool(torch.isneginf(s).all()) and bool((i == -1).all())
    s, i = ops.dot_topk_fp8(q[:0], torch.zeros(9, 128, dtype=torch.uint8, device=dev), torch.ones(9, device=dev), 5)
    assert s.shape == i.shape == (0, 5)


def test_operator_refuses_wrong_dtypes_and_mismatched_shapes():
    from matchmaker_amd import NativeError, _lib, ops
    dev = util.require_gpu()
    q = torch.zeros(2, 128, dtype=torch.float16, device=dev)
    codes = torch.zeros(5, 128, dtype=torch.uint8, device=dev)
    scales = torch.ones(5, device=dev)
    with pytest.raises(NativeError, match="fp16 or bf16") as e:
        ops.dot_topk_fp8(q.float(), codes, scales, 3)
    assert e.value.code == _lib.MM_EUNSUPPORTED
    with pytest.raises(NativeError, match="uint8"):
        ops.dot_topk_fp8(q, codes.half(), scales, 3)
    with pytest.raises(NativeError, match="scales"):
        ops.dot_topk_fp8(q, codes, scales[:4], 3)
    with pytest.raises(NativeError, match="embedding dims differ"):
        ops.dot_topk_fp8(q[:, :64], codes, scales, 3)
    with pytest.raises(NativeError) as e:                                  # a width the kernel is not instantiated for
        ops.dot_topk_fp8(q[:, :64].contiguous(), codes[:, :64].contiguous(), scales, 3)
    assert e.value.code == _lib.MM_EUNSUPPORTED and "pad the vectors" in str(e.value)
    with pytest.raises(NativeError) as e:
        ops.dot_topk_fp8(q, codes, scales, 4097)
    assert e.value.code == _lib.MM_EUNSUPPORTED


# ---- determinism -------------------------------------------------------------------------------------------------------

def test_two_calls_are_bit_equal_and_a_row_does_not_depend_on_its_batch():
    q, codes, scales = R.scaled_store(257, 20000, 256, 179)
    a = _search(q, codes, scales, 100)
    b = _search(q, codes, scales, 100)
    _equal(b, a, "second call")
    one = _search(q[:1], codes, scales, 100)            # one query tile alone against two tiles with a partial group
    _equal(one, (a[0][:1], a[1][:1]), "nq = 1 against row 0 of nq = 257")
    _equal(a, R.dot_topk_fp8_exact(q, codes, scales, 100), "reference")
    # random data too: not exact, but the same bits whatever the batch
    q, codes, scales = R.random_inputs("bfloat16", 128, 70001, nq=257)
    a = _search(q, codes, scales, 50, "bfloat16")
    _equal(_search(q, codes, scales, 50, "bfloat16"), a, "random: second call")
    _equal(_search(q[:1], codes, scales, 50, "bfloat16"), (a[0][:1], a[1][:1]), "random: nq = 1 against row 0 of nq = 257")


# ---- TokenStore end to end ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _exact_reference():
    """colbert_search_reference.exact_case() and the restatement's results on it: computed once, never modified"""
    c = CR.exact_case()
    hits = CR.token_hits_ref(c["q"], c["tokens"], c["k"])
    ref = {sr: CR.search_ref(c["q"], c["tokens"], c["begin"], c["end"], c["k"], c["top_n"], sim_round=sr, hit_rows=hits)
           for sr in (True, False)}
    return c, hits, ref


def test_fp8_only_store_retrieves_end_to_end(tmp_path):
    from matchmaker_amd import NativeError, _lib
    from matchmaker_amd.token_store import TokenStore
    dev = util.require_gpu()
    c, hits_ref, ref = _exact_reference()
    ids = [f"doc{i}" for i in range(len(c["begin"]))]
    st16 = TokenStore(torch.from_numpy(c["tokens"]).half().to(dev), ids, c["begin"], c["end"])
    st16.quantize_fp8().save_fp8(str(tmp_path / "fp8"))
    only = TokenStore.load_fp8(str(tmp_path / "fp8"), dev)                 # an fp8-ONLY store: no 16-bit rows anywhere
    assert only.is_fp8 and only._tokens is None
    assert np.array_equal(F.dequantize_numpy(only.codes.cpu().numpy(), only.scales.cpu().numpy()), c["tokens"].astype(np.float64))
    q = torch.from_numpy(c["q"]).half().to(dev)
    with pytest.raises(NativeError, match="holds no 16-bit rows") as ei:   # without the option: as before
        only.token_hits(q, c["k"])
    assert ei.value.code == _lib.MM_EUNSUPPORTED
    for shard in (None, 64, 1024):
        hits = only.token_hits(q, c["k"], token_search="fp8", row_shard=shard)
        np.testing.assert_array_equal(hits.cpu().numpy(), hits_ref, err_msg=f"row_shard = {shard}")
        np.testing.assert_array_equal(st16.token_hits(q, c["k"], row_shard=shard).cpu().numpy(), hits_ref)
        for use_fp16 in (True, False):
            s, d = only.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16, token_search="fp8", row_shard=shard)
            np.testing.assert_array_equal(d.cpu().numpy(), ref[use_fp16][1])
            np.testing.assert_array_equal(s.cpu().numpy(), ref[use_fp16][0])
            s16, d16 = st16.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16, row_shard=shard)
            assert torch.equal(s, s16) and torch.equal(d, d16)             # bit for bit the 16-bit store's search
            res = only.search(q, c["top_n"], c["k"], use_fp16=use_fp16, token_search="fp8", row_shard=shard)
            assert res == [[(ids[j], float(x)) for x, j in zip(si, di) if j >= 0]
                           for si, di in zip(s.cpu().tolist(), d.cpu().tolist())]
