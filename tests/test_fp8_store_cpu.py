"""CPU tests of the fp8 ColBERT token store: the C ABI declarations and the binding, the torch ops' fake rules, the properties
of the restated format (element bound, scaled maximum, no NaN code, idempotence), the score bound, and TokenStore's fp8 host
logic driven through stand-ins for the native calls."""
import os

import numpy as np
import pytest
import torch

from tests import fp8_store_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


# ------------------------------------------------------------------------------------------ C ABI, binding, torch ops
def test_header_and_binding_declare_the_three_entry_points():
    from matchmaker_amd import _lib, build
    from tests import abi
    L = abi.assert_bound(("mm_fp8_quantize_rows", "mm_maxsim_ragged_fp8_workspace_bytes", "mm_maxsim_ragged_fp8_fwd"))
    hdr = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    assert "e4m3fn" in hdr and "fnuz" in hdr
    assert "maxsim_fp8.hip" in build.SOURCES
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    # host arithmetic and refusals: callable without a GPU, nothing is launched
    assert L.mm_maxsim_ragged_fp8_workspace_bytes(10, 1, 32, _lib.MASK_NONE) == 0
    assert L.mm_maxsim_ragged_fp8_workspace_bytes(10, 5, 32, _lib.MASK_U8) > 0
    p = 4096                                                               # any non-null aligned value: refused before it is used
    assert L.mm_fp8_quantize_rows(p, 4, 24, _lib.MM_F16, p, p, None) == _lib.MM_EUNSUPPORTED
    assert L.mm_fp8_quantize_rows(p, 4, 32, 7, p, p, None) == _lib.MM_EINVAL
    assert L.mm_fp8_quantize_rows(p, 0, 32, _lib.MM_F16, p, p, None) == _lib.MM_OK
    args = (p, p, p, p, p, None, _lib.MASK_NONE, p, 4, 1, 32)
    assert L.mm_maxsim_ragged_fp8_fwd(*args, 128, _lib.MM_F32, 0, None, 0, None) == _lib.MM_EUNSUPPORTED
    assert b"fp16 or bf16" in L.mm_last_error()
    assert L.mm_maxsim_ragged_fp8_fwd(*args, 40, _lib.MM_BF16, 0, None, 0, None) == _lib.MM_EUNSUPPORTED
    assert L.mm_maxsim_ragged_fp8_fwd(*args, 128, _lib.MM_BF16, 4, None, 0, None) == _lib.MM_EINVAL
    assert L.mm_maxsim_ragged_fp8_fwd(p, p, p, p, p, None, _lib.MASK_NONE, p, 0, 1, 32, 128, _lib.MM_BF16, 0, None, 0, None) == _lib.MM_OK


def test_ops_refuse_cpu_tensors_and_export_the_names():
    import matchmaker_amd
    from matchmaker_amd import ops, NativeError
    assert matchmaker_amd.fp8_quantize_rows is ops.fp8_quantize_rows and matchmaker_amd.maxsim_ragged_fp8 is ops.maxsim_ragged_fp8
    assert matchmaker_amd.fp8_dequantize_rows is ops.fp8_dequantize_rows
    from matchmaker_amd.token_store import TokenStore
    assert matchmaker_amd.TokenStore is TokenStore
    with pytest.raises(NativeError, match="CPU"):
        ops.fp8_quantize_rows(torch.zeros(4, 16))
    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(NativeError, match="CPU"):
        ops.maxsim_ragged_fp8(torch.zeros(2, 4, 16, dtype=torch.float16), torch.zeros(8, 16, dtype=torch.uint8), torch.ones(8), z, z)


@pytest.mark.parametrize("T, E, dtype", [(4097, 128, torch.float16), (1, 16, torch.float32), (0, 768, torch.bfloat16)])
def test_fake_rule_of_the_quantiser(T, E, dtype):
    from matchmaker_amd import torch_ops  # noqa: F401
    codes, scales = torch.ops.mm_native.fp8_quantize_rows(torch.empty(T, E, dtype=dtype, device="meta"))
    assert codes.shape == (T, E) and codes.dtype == torch.uint8 and scales.shape == (T,) and scales.dtype == torch.float32
    assert codes.device.type == "meta" and not codes.requires_grad


@pytest.mark.parametrize("n_pairs, ppq", [(12, 1), (12, 7), (0, 3)])
def test_fake_rule_of_the_maxsim(n_pairs, ppq):
    from matchmaker_amd import torch_ops  # noqa: F401
    nq = (n_pairs + ppq - 1) // ppq
    m = dict(device="meta")
    out = torch.ops.mm_native.maxsim_ragged_fp8(torch.empty(nq, 32, 128, dtype=torch.bfloat16, **m), torch.empty(500, 128, dtype=torch.uint8, **m),
                                                torch.empty(500, **m), torch.empty(n_pairs, dtype=torch.int64, **m),
                                                torch.empty(n_pairs, dtype=torch.int64, **m), None, ppq, False, True)
    assert out.shape == (n_pairs,) and out.dtype == torch.float32 and out.device.type == "meta"


# ------------------------------------------------------------------------------------------ the restated format
@pytest.mark.parametrize("dtype", DTYPES)
def test_restatement_properties_on_seeded_rows(dtype):
    """T = 4097 rows of mixed magnitude with the special rows: the element bound |deq s - x| <= 2^-4 |x| + 2^-10 s, the scaled
    maximum in [128, 256), no NaN code, power-of-two scales, and the numpy restatement equal to the torch one."""
    x = R.special_rows(4097, 128, dtype, seed=3)
    codes, s = R.quantize_torch(x)
    xf = x.float()
    assert codes.dtype == torch.uint8 and s.dtype == torch.float32 and codes.shape == x.shape and s.shape == (4097,)
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all())                                          # powers of two
    assert not bool(((codes & 0x7f) == 0x7f).any())                        # 0x7f / 0xff never appear
    a = xf.abs().amax(dim=1)
    zero = a == 0
    assert bool(zero[1]) and bool((s[zero] == 1).all()) and bool((R.fold_zero(codes[zero]) == 0).all())
    if dtype == torch.float16:
        assert bool(zero[3])                                               # 1e-30 underflows fp16: a zero row there
    else:
        assert not bool(zero[3]) and float(s[3]) < 2.0 ** -90
    scaled_max = (a / s)[~zero]
    assert bool((scaled_max >= 128).all()) and bool((scaled_max < 256).all())
    assert float(a[4]) == 1.0 and float(s[4]) == 2.0 ** -7                 # an exact power of two sits at 128
    deq = R.dequantize_torch(codes, s).double()
    err = (deq - xf.double()).abs()
    lim = 2.0 ** -4 * xf.double().abs() + 2.0 ** -10 * s.double()[:, None]
    assert bool((err <= lim).all())
    worst = float((err / lim.clamp_min(1e-300)).max())
    print(f"{dtype}: worst element error / bound = {worst:.3f}")
    assert worst > 0.5                                                     # the bound is not slack by construction
    # -0.0 elements: a zero either way
    assert bool((R.fold_zero(codes[2, ::2]) == 0).all())
    # numpy restatement, codes with the zeros folded, and the dequantiser tables
    cn, sn = R.quantize_numpy(xf.numpy())
    assert np.array_equal(sn, s.numpy()) and np.array_equal(R.fold_zero(cn), R.fold_zero(codes).numpy())
    assert np.array_equal(R.dequantize_numpy(codes.numpy(), s.numpy()), deq.numpy())


def test_e4m3fn_table_equals_torch_cast():
    c = torch.arange(256, dtype=torch.uint8)
    t = c.view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(np.isnan(t), np.isnan(R.E4M3)) and np.array_equal(t[~np.isnan(t)], R.E4M3[~np.isnan(t)])
    assert np.isnan(R.E4M3[[0x7f, 0xff]]).all() and R.E4M3[0x7e] == 448 and R.E4M3[0x01] == 2.0 ** -9 and R.E4M3[0x70] == 128
    ok = ~np.isnan(R.E4M3) & (np.abs(np.nan_to_num(R.E4M3)) < 256)
    assert np.array_equal(R.fold_zero(R.encode_e4m3fn_numpy(R.E4M3[ok])), R.fold_zero(np.arange(256, dtype=np.uint8)[ok]))
    # ties go to even: halfway between 16 (0x58) and 18 (0x59), and between 18 and 20 (0x5a)
    assert R.encode_e4m3fn_numpy(np.array([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10])).tolist() == [0x58, 0x5a, 0x00, 0x02]


def test_quantising_a_dequantised_store_returns_it():
    """quantize(deq(c) s) == (c, s) for rows whose largest code magnitude lies in [128, 256) (codes 0x70 .. 0x77)."""
    rng = np.random.default_rng(11)
    T, E = 4097, 48
    mag = rng.integers(0, 0x78, (T, E))
    mag[np.arange(T), rng.integers(0, E, T)] = rng.integers(0x70, 0x78, T)
    codes = (mag | (rng.integers(0, 2, (T, E)) << 7)).astype(np.uint8)
    scales = np.ldexp(np.float32(1), rng.integers(-100, 100, T)).astype(np.float32)
    x = R.dequantize_numpy(codes, scales).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), R.dequantize_numpy(codes, scales))      # the product is exact in fp32
    c2, s2 = R.quantize_torch(torch.from_numpy(x))
    assert np.array_equal(s2.numpy(), scales) and np.array_equal(R.fold_zero(c2.numpy()), R.fold_zero(codes))
    c3, s3 = R.quantize_numpy(x)
    assert np.array_equal(s3, scales) and np.array_equal(R.fold_zero(c3), R.fold_zero(codes))


def test_clamped_scales_at_the_ends_of_the_float32_range():
    x = torch.zeros(3, 16)
    x[0, 0] = 2.0 ** -140                                                  # subnormal maximum: k = -126
    x[1, 0] = 3.0e38                                                       # k = 127 - 7 = 120
    x[2, 0] = 2.0 ** -119                                                  # floor(log2) - 7 = -126, the last unclamped one
    codes, s = R.quantize_torch(x)
    assert s.tolist() == [2.0 ** -126, 2.0 ** 120, 2.0 ** -126]
    assert R.E4M3[int(codes[2, 0])] == 128 and 128 <= R.E4M3[int(codes[1, 0])] < 256 and int(codes[0, 0]) == 0


def test_score_bound_of_the_quantised_store_on_the_restatement():
    """|fp8 score - 16-bit score| <= sum_i max_t sum_k |q_ik| (2^-4 |x_tk| + 2^-10 s_t) on unit-normalised random rows."""
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 90, 40)
    end = np.cumsum(lens)
    begin = end - lens
    x = rng.standard_normal((int(end[-1]), 128))
    x = torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(torch.bfloat16)
    q = rng.standard_normal((4, 32, 128))
    q = torch.from_numpy(q / np.linalg.norm(q, axis=2, keepdims=True)).to(torch.bfloat16).double().numpy()
    codes, s = R.quantize_torch(x)
    codes, s = codes.numpy(), s.numpy()
    fp8 = R.maxsim_ragged_fp8_ref(q, codes, s, begin, end, pairs_per_query=10)
    x64 = x.double().numpy()
    worst = 0.0
    for p in range(40):
        qi = q[p // 10]
        full = (x64[begin[p]: end[p]] @ qi.T).max(axis=0).sum()
        lim = ((2.0 ** -4 * np.abs(x64[begin[p]: end[p]]) + 2.0 ** -10 * s[begin[p]: end[p], None].astype(np.float64)) @ np.abs(qi).T).max(axis=0).sum()
        assert abs(fp8[p] - full) <= lim
        worst = max(worst, abs(fp8[p] - full) / lim)
    print(f"worst score change / bound = {worst:.3f}")
    # an empty range scores -1000 per live token, with and without a mask
    mask = np.ones((1, 32), dtype=bool)
    mask[0, 5] = False
    assert R.maxsim_ragged_fp8_ref(q[:1], codes, s, [3], [3]).tolist() == [-32000.0]
    assert R.maxsim_ragged_fp8_ref(q[:1], codes, s, [3], [3], q_mask=mask, flags=1, q_dtype=torch.float16).tolist() == [-31000.0]
    # MM_SUM_ROUND: fp16 has steps of 16 there
    assert R.maxsim_ragged_fp8_ref(q[:1], codes, s, [3], [3], q_mask=mask, flags=3, q_dtype=torch.float16).tolist() == [-31008.0]


@pytest.mark.parametrize("Q, E", [(65, 768), (64, 768), (33, 256), (1, 48)])
def test_exact_case_is_exact_in_fp32(Q, E):
    """The premise of the GPU suite's bit-equal test: every product is an integer of magnitude <= 16, so every partial sum of
    a similarity is an integer below E * 16 < 2^24; the scaled similarities are multiples of 1/8, and the sum of the
    magnitudes of a pair's Q maxima, in eighths, stays below 2^24 — so the sum over query tokens is exact in any order."""
    for ppq in (1, 7):
        c = R.exact_case(Q, E, ppq, seed=1000 * Q + E + ppq)
        assert sorted((c["end"] - c["begin"]).tolist()) == R.EXACT_LENS and int(c["end"].max()) == c["T"] == sum(R.EXACT_LENS)
        assert c["nq"] == (12 if ppq == 1 else 2) and np.abs(R.deq_numpy(c["codes"])).max() <= 8 and np.abs(c["q"]).max() <= 2
        assert set(np.log2(c["scales"]).tolist()) <= set(range(-3, 4)) and E * 16 < 2 ** 24
        for _, mx, _ in R._token_maxima(c["q"], c["codes"], c["scales"], c["begin"], c["end"], ppq):
            if mx is not None:
                assert np.array_equal(mx * 8, np.round(mx * 8)) and np.abs(mx).sum() * 8 < 2 ** 24
                assert np.abs(mx).max() < 65504                           # MM_SIM_ROUND to fp16 stays finite


# ------------------------------------------------------------------------------------------ TokenStore through stand-ins
class _Fp8StandIns:
    def __init__(self):
        self.calls = []

    def quantize(self, x):
        self.calls.append(("quantize", tuple(x.shape), x.dtype))
        return R.quantize_torch(x)

    def maxsim(self, q, codes, scales, b, e, q_mask, pairs_per_query, check_ranges, sim_round):
        assert q_mask is None and check_ranges is False and codes.dtype == torch.uint8 and scales.dtype == torch.float32
        self.calls.append(("maxsim", q.dtype, pairs_per_query, sim_round, b.tolist(), e.tolist()))
        ref = R.maxsim_ragged_fp8_ref(q.double().numpy(), codes.numpy(), scales.numpy(), b.tolist(), e.tolist(),
                                      pairs_per_query=pairs_per_query, flags=R.SIM_ROUND if sim_round else 0, q_dtype=q.dtype)
        return torch.from_numpy(ref).float()


def _small_store(fn, dtype=torch.float16):
    from matchmaker_amd.token_store import TokenStore
    rng = np.random.default_rng(2)
    lens = [3, 0, 5, 2, 7]
    end = np.cumsum(lens)
    begin = end - lens
    tokens = torch.from_numpy(rng.integers(-16, 17, (int(end[-1]), 16)) / 8.0).to(dtype)
    tokens[tokens.abs().sum(-1) == 0, 0] = 0.125
    ids = [f"d{i}" for i in range(5)]
    return TokenStore(tokens, ids, begin, end, quantize_fn=fn.quantize), tokens, ids, begin, end


def test_quantize_fp8_makes_an_fp8_store():
    from matchmaker_amd import NativeError
    fn = _Fp8StandIns()
    st, tokens, ids, begin, end = _small_store(fn)
    assert not st.is_fp8
    with pytest.raises(NativeError, match="not an fp8 store"):
        st.codes
    f8 = st.quantize_fp8(maxsim_fn=fn.maxsim)
    assert fn.calls[0] == ("quantize", (17, 16), torch.float16)
    assert f8.is_fp8 and f8.codes.shape == (17, 16) and f8.codes.dtype == torch.uint8 and f8.scales.shape == (17,)
    assert torch.equal(R.dequantize_torch(f8.codes, f8.scales, torch.float16), tokens)      # multiples of 1/8 up to 2: lossless
    assert f8.seq_ids == ids and f8._begin.tolist() == begin.tolist() and f8._begin_sorted.tolist() == [0, 3, 8, 10]
    with pytest.raises(NativeError, match="keep_tokens=True"):
        f8.tokens
    with pytest.raises(NativeError, match="already"):
        f8.quantize_fp8()
    kept = st.quantize_fp8(keep_tokens=True, maxsim_fn=fn.maxsim)
    assert kept.is_fp8 and kept.tokens is st.tokens
    with pytest.raises(NativeError, match="uint8"):
        type(st)(None, ids, begin, end, codes=f8.codes.float(), scales=f8.scales)
    with pytest.raises(NativeError, match="leave the 17-row"):
        type(st)(None, ids, begin, end + 1, codes=f8.codes, scales=f8.scales)
    with pytest.raises(NativeError, match="codes \\+ scales"):
        type(st)(None, ids, begin, end)


def test_token_hits_of_an_fp8_store_needs_an_index_or_the_kept_rows():
    from matchmaker_amd import NativeError, _lib
    fn = _Fp8StandIns()
    st, tokens, *_ = _small_store(fn)
    f8 = st.quantize_fp8(maxsim_fn=fn.maxsim)
    q = torch.ones(1, 2, 16)
    with pytest.raises(NativeError, match="index=.*keep_tokens=True") as ei:
        f8.token_hits(q, 2)
    assert ei.value.code == _lib.MM_EUNSUPPORTED
    with pytest.raises(NativeError, match="keep_tokens=True"):
        f8.search_device(q, 3, 2)

    class _Index:                                                          # an indexer that holds its own vectors
        def search_device(self, qs, k):
            assert qs.dtype == torch.float16
            return None, torch.arange(k).repeat(qs.shape[0], 1)

    assert f8.token_hits(q, 2, index=_Index()).tolist() == [[0, 1, 0, 1]]


@pytest.mark.parametrize("src, use_fp16, want_q", [(torch.float16, True, torch.float16), (torch.float16, False, torch.float16),
                                                    (torch.bfloat16, True, torch.float16), (torch.bfloat16, False, torch.bfloat16),
                                                    (torch.float32, False, torch.bfloat16)])
def test_aggregate_pads_lists_and_picks_the_query_dtype(src, use_fp16, want_q):
    fn = _Fp8StandIns()
    st, tokens, ids, begin, end = _small_store(fn, src)
    f8 = st.quantize_fp8(maxsim_fn=fn.maxsim)
    q = torch.from_numpy(np.random.default_rng(4).integers(-2, 3, (2, 3, 16)).astype(np.float32))
    out = f8.aggregate(q, [["d4", "d0", "d1"], ["d2"]], use_fp16=use_fp16)
    kind, qd, ppq, sim_round, b, e = fn.calls[-1]
    assert (kind, qd, ppq, sim_round) == ("maxsim", want_q, 3, use_fp16)
    assert b == [10, 0, 3, 3, 0, 0] and e == [17, 3, 3, 8, 0, 0]           # the short list padded with empty ranges
    assert [[i for i, _ in r] for r in out] == [["d4", "d0", "d1"], ["d2"]]
    t64 = tokens.double().numpy()
    for i, r in enumerate(out):
        for sid, sc in r:
            j = ids.index(sid)
            want = (q[i].double().numpy() @ t64[begin[j]: end[j]].T).max(-1).sum() if end[j] > begin[j] else -3000.0
            assert sc == want                                              # small integers / 8: exact, fp16 rounding included
    assert f8.aggregate(q, [[], []]) == [[], []]


def test_save_fp8_load_fp8_round_trip(tmp_path):
    from matchmaker_amd import NativeError
    from matchmaker_amd.token_store import TokenStore
    fn = _Fp8StandIns()
    st, tokens, ids, begin, end = _small_store(fn, torch.bfloat16)
    with pytest.raises(NativeError, match="not an fp8 store"):
        st.save_fp8(str(tmp_path / "x"))
    f8 = st.quantize_fp8(maxsim_fn=fn.maxsim)
    f8.save_fp8(str(tmp_path / "store"))
    assert sorted(os.listdir(tmp_path / "store")) == ["codes.npy", "docs.npz", "scales.npy"]
    back = TokenStore.load_fp8(str(tmp_path / "store"), "cpu", maxsim_fn=fn.maxsim)
    assert back.is_fp8 and torch.equal(back.codes, f8.codes) and torch.equal(back.scales, f8.scales)
    assert back.seq_ids == ids and back._begin.tolist() == begin.tolist() and back._end.tolist() == end.tolist()
    assert back._source_dtype == torch.bfloat16
    q = torch.ones(1, 2, 16)
    assert back.aggregate(q, [ids], use_fp16=False) == f8.aggregate(q, [ids], use_fp16=False)
    assert fn.calls[-1][1] == torch.bfloat16


def test_load_fp8_true_quantises_file_by_file(tmp_path):
    """A folder written by write_reference_store with two files: load(..., fp8=True) quantises each file on its own and the
    result equals the quantised 16-bit store."""
    from matchmaker_amd.token_store import TokenStore, write_reference_store
    rng = np.random.default_rng(8)
    docs = [rng.standard_normal((n, 16)).astype(np.float16) for n in (5, 9, 4, 7, 6)]
    ids = [f"s{i}" for i in range(5)]
    write_reference_store(str(tmp_path), docs, ids, token_block_size=20, token_dtype="float16")
    assert len([f for f in os.listdir(tmp_path) if f.startswith("token_reps_")]) == 2
    fn = _Fp8StandIns()
    f8 = TokenStore.load(str(tmp_path), 16, "float16", 20, "cpu", fp8=True, quantize_fn=fn.quantize, maxsim_fn=fn.maxsim)
    assert [c[1] for c in fn.calls if c[0] == "quantize"] == [(18, 16), (13, 16)]      # one call per file, never the whole store
    st = TokenStore.load(str(tmp_path), 16, "float16", 20, "cpu")
    codes, scales = R.quantize_torch(st.tokens)
    assert f8.is_fp8 and torch.equal(f8.codes, codes) and torch.equal(f8.scales, scales) and f8._source_dtype == torch.float16
    assert f8._begin.tolist() == st._begin.tolist() and f8._end.tolist() == st._end.tolist() and f8.seq_ids == st.seq_ids
    with pytest.raises(Exception, match="keep_tokens=True"):
        f8.tokens
    q = torch.from_numpy(rng.standard_normal((1, 4, 16)).astype(np.float32))
    got = f8.aggregate(q, [ids])
    want = R.maxsim_ragged_fp8_ref(q.half().double().numpy(), codes.numpy(), scales.numpy(), st._begin.tolist(), st._end.tolist(),
                                   pairs_per_query=5, flags=R.SIM_ROUND, q_dtype=torch.float16)
    assert [s for _, s in got[0]] == [float(np.float32(w)) for w in want]
