"""GPU tests of the fp8 ColBERT token store: the quantiser kernel bit for bit against the restatement, the ragged MaxSim on
exactly representable arithmetic (bit-equal to the float64 restatement) and on random data (within the fp32 accumulation
bound), edges and refusals, TokenStore in fp8 mode, and graph replay of the ranking chain."""
import functools

import numpy as np
import pytest
import torch

from tests import colbert_search_reference as CR
from tests import fp8_store_reference as R
from tests import util

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]


# ------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("E", [16, 128, 768])
@pytest.mark.parametrize("T", [1, 33, 4097])
def test_quantiser_is_bit_equal_to_the_restatement(T, E, dtype):
    """Codes (the two zeros folded) and scales equal the torch restatement on rows of mixed magnitude, a zero row, -0.0
    elements, a row scaled by 1e-30 and maxima at and just below a power of two; a second call gives the same bits."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    x = R.special_rows(T, E, dtype, seed=100 + E)
    want_c, want_s = R.quantize_torch(x)
    codes, scales = ops.fp8_quantize_rows(x.to(dev))
    assert codes.shape == (T, E) and codes.dtype == torch.uint8 and scales.shape == (T,) and scales.dtype == torch.float32
    assert torch.equal(scales.cpu(), want_s)
    assert torch.equal(R.fold_zero(codes.cpu()), R.fold_zero(want_c))
    c2, s2 = ops.fp8_quantize_rows(x.to(dev))
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    # the plain-torch dequantiser on the device equals the restated one
    assert torch.equal(ops.fp8_dequantize_rows(codes, scales, torch.float32).cpu(), R.dequantize_torch(want_c, want_s))


def test_quantiser_of_a_strided_view_and_of_no_rows():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    x = R.special_rows(40, 64, torch.float16, seed=1).to(dev)
    view = x[:, :32]                                                       # not contiguous: quantised as its own [40, 32] matrix
    c, s = ops.fp8_quantize_rows(view)
    wc, ws = R.quantize_torch(view.cpu())
    assert torch.equal(R.fold_zero(c.cpu()), R.fold_zero(wc)) and torch.equal(s.cpu(), ws)
    c0, s0 = ops.fp8_quantize_rows(x[:0])
    assert c0.shape == (0, 64) and s0.shape == (0,)


# ------------------------------------------------------------------------------------------ MaxSim, exact arithmetic
@pytest.mark.parametrize("E", [128, 256, 768, 48])
@pytest.mark.parametrize("Q", [1, 32, 33, 64, 65])
def test_maxsim_is_bit_equal_on_exactly_representable_data(Q, E):
    """Integer codes in -8..8, scales 2^-3..2^3, integer queries in -2..2: every similarity and every sum is exact in fp32,
    so the kernel equals the float64 restatement bit for bit — document lengths 0 .. 200 around the 32- and 64-row block
    edges (the last document ends at row T), pairs_per_query 1 and 7 (a short last query), both query dtypes, flags 0 /
    SIM_ROUND / SIM_ROUND | SUM_ROUND, with and without a q_mask with a hole.  E = 48 and Q = 65 take the plain kernel,
    E = 768 with Q > 32 the 32-row ring."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    for ppq in (1, 7):
        c = R.exact_case(Q, E, ppq, seed=1000 * Q + E + ppq)
        assert int(c["end"].max()) == c["T"] and sorted((c["end"] - c["begin"]).tolist()) == R.EXACT_LENS
        codes, scales = torch.from_numpy(c["codes"]).to(dev), torch.from_numpy(c["scales"]).to(dev)
        b, e = torch.from_numpy(c["begin"]).to(dev), torch.from_numpy(c["end"]).to(dev)
        for qd in (torch.bfloat16, torch.float16):
            q = torch.from_numpy(c["q"]).to(qd).to(dev)
            for flags in (0, R.SIM_ROUND, R.SIM_ROUND | R.SUM_ROUND):
                for mask in (None, c["mask"]):
                    ref = R.maxsim_ragged_fp8_ref(c["q"], c["codes"], c["scales"], c["begin"], c["end"], q_mask=mask,
                                                  pairs_per_query=ppq, flags=flags, q_dtype=qd)
                    got = ops.maxsim_ragged_fp8(q, codes, scales, b, e, None if mask is None else torch.from_numpy(mask).to(dev),
                                                pairs_per_query=ppq, sim_round=bool(flags & 1), sum_round=bool(flags & 2))
                    assert got.dtype == torch.float32 and got.shape == (c["n_pairs"],)
                    assert np.array_equal(got.cpu().double().numpy(), ref), (ppq, qd, flags, mask is not None)


# ------------------------------------------------------------------------------------------ MaxSim, random data
@functools.lru_cache(maxsize=None)
def _random_case(kind, Q, E):
    rng = np.random.default_rng(7 + Q + E)
    lens = rng.integers(0, 150, 48)
    lens[-1] = 77
    end = np.cumsum(lens).astype(np.int64)
    begin = end - lens
    T = int(end[-1])
    x = rng.standard_normal((T, E)).astype(np.float32)
    if kind == "unit":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    else:                                                                  # rows of mixed magnitude
        x *= np.exp2(rng.integers(-10, 6, (T, 1))).astype(np.float32)
    q = rng.standard_normal((6, Q, E)).astype(np.float32)
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    codes, scales = R.quantize_torch(torch.from_numpy(x).to(torch.bfloat16))
    q16 = torch.from_numpy(q).to(torch.bfloat16)
    ref = R.maxsim_ragged_fp8_ref(q16.double().numpy(), codes.numpy(), scales.numpy(), begin, end, pairs_per_query=8)
    lim = R.bound(q16.double().numpy(), codes.numpy(), scales.numpy(), begin, end, ref, pairs_per_query=8)
    return q16, codes, scales, begin, end, ref, lim


@pytest.mark.parametrize("Q, E", [(32, 128), (40, 256), (50, 768), (32, 80)])
@pytest.mark.parametrize("kind", ["unit", "mixed"])
def test_maxsim_on_random_data_is_within_the_accumulation_bound(kind, Q, E):
    """|kernel - float64 restatement| <= (E + Q + 2) 2^-24 sum_i max_t s_t sum_k |q_ik| |deq_tk| per pair, and within twice
    that of ops.maxsim_ragged on the bf16 dequantised matrix (the same exact products, summed by another kernel).  flags 0:
    with a rounding flag a maximum a hair from an fp16 tie may round the other way, which the exact-data test covers
    instead."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q16, codes, scales, begin, end, ref, lim = _random_case(kind, Q, E)
    b, e = torch.from_numpy(begin).to(dev), torch.from_numpy(end).to(dev)
    got = ops.maxsim_ragged_fp8(q16.to(dev), codes.to(dev), scales.to(dev), b, e, pairs_per_query=8).cpu().double().numpy()
    err = np.abs(got - ref)
    print(f"{kind} Q{Q} E{E}: worst error / bound = {float((err / np.maximum(lim, 1e-300)).max()):.3f}")
    assert (err <= lim).all()
    deq16 = R.dequantize_torch(codes, scales, torch.bfloat16)
    assert torch.equal(deq16.float(), R.dequantize_torch(codes, scales))   # the dequantised matrix is exact in bf16
    other = ops.maxsim_ragged(q16.to(dev), deq16.to(dev), b, e, pairs_per_query=8).cpu().double().numpy()
    assert (np.abs(got - other) <= 2 * lim).all()


# ------------------------------------------------------------------------------------------ edges and errors
def test_no_pairs_and_all_ranges_empty():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    c = R.exact_case(33, 128, 1, seed=4)
    codes, scales = torch.from_numpy(c["codes"]).to(dev), torch.from_numpy(c["scales"]).to(dev)
    q = torch.from_numpy(c["q"]).to(torch.float16).to(dev)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    assert ops.maxsim_ragged_fp8(q[:0], codes, scales, none, none).shape == (0,)
    at = torch.tensor([0, 5, c["T"], 17], dtype=torch.int64, device=dev)   # empty ranges anywhere in [0, T]
    mask = torch.from_numpy(c["mask"][:4]).to(dev)
    live = mask.sum(dim=1).float()
    for E_codes, E_scales, qq in ((codes, scales, q), (codes[:, :48].contiguous(), scales, q[:, :, :48].contiguous())):
        out = ops.maxsim_ragged_fp8(qq[:4], E_codes, E_scales, at, at)
        assert out.tolist() == [-33000.0] * 4
        out = ops.maxsim_ragged_fp8(qq[:4], E_codes, E_scales, at, at, q_mask=mask)
        assert torch.equal(out, -1000.0 * live)
    out = ops.maxsim_ragged_fp8(q[:2], codes, scales, at, at, pairs_per_query=2, sim_round=True, sum_round=True)
    assert out.tolist() == [float(np.float16(-33000.0))] * 4


def test_every_refusal_is_a_native_error():
    from matchmaker_amd import ops, NativeError, _lib
    dev = util.require_gpu()
    codes = torch.zeros(64, 128, dtype=torch.uint8, device=dev)
    scales = torch.ones(64, device=dev)
    q = torch.zeros(2, 8, 128, dtype=torch.bfloat16, device=dev)
    b = torch.tensor([0, 10], dtype=torch.int64, device=dev)
    e = torch.tensor([10, 64], dtype=torch.int64, device=dev)
    assert ops.maxsim_ragged_fp8(q, codes, scales, b, e).tolist() == [0.0, 0.0]
    with pytest.raises(NativeError, match="fp16 or bf16") as ei:
        ops.maxsim_ragged_fp8(q.float(), codes, scales, b, e)
    assert ei.value.code == _lib.MM_EUNSUPPORTED
    with pytest.raises(NativeError, match="uint8"):
        ops.maxsim_ragged_fp8(q, codes.to(torch.int8), scales, b, e)
    with pytest.raises(NativeError, match="uint8"):
        ops.maxsim_ragged_fp8(q, codes.to(torch.bfloat16), scales, b, e)
    with pytest.raises(NativeError, match=r"scales: expected \[64\]"):
        ops.maxsim_ragged_fp8(q, codes, scales[:63], b, e)
    with pytest.raises(NativeError, match="float32"):
        ops.maxsim_ragged_fp8(q, codes, scales.double(), b, e)
    with pytest.raises(NativeError, match="multiple of 16") as ei:
        ops.maxsim_ragged_fp8(q[:, :, :40].contiguous(), codes[:, :40].contiguous(), scales, b, e)
    assert ei.value.code == _lib.MM_EUNSUPPORTED
    with pytest.raises(NativeError, match="multiple of 16"):
        ops.fp8_quantize_rows(torch.zeros(4, 24, dtype=torch.float16, device=dev))
    with pytest.raises(NativeError, match="dims differ"):
        ops.maxsim_ragged_fp8(q[:, :, :64].contiguous(), codes, scales, b, e)
    with pytest.raises(NativeError, match="pairs"):
        ops.maxsim_ragged_fp8(q, codes, scales, b, e, pairs_per_query=3)
    # a range past T is refused under check_ranges (and only there: the kernel does not know T)
    with pytest.raises(NativeError, match="leave the 64-row"):
        ops.maxsim_ragged_fp8(q, codes, scales, b, e + 1)
    with pytest.raises(NativeError, match="begin > end"):
        ops.maxsim_ragged_fp8(q, codes, scales, e, b)
    with pytest.raises(NativeError, match="leave the 64-row"):
        ops.maxsim_ragged_fp8(q, codes, scales, b - 1, e)


# ------------------------------------------------------------------------------------------ TokenStore
@functools.lru_cache(maxsize=None)
def _exact_stores():
    """The exact store of the end-to-end tests (multiples of 1/8 up to 2: its quantisation is lossless), the restatement's
    results (computed once, never modified), the 16-bit store over the dequantised matrix and the fp8 store."""
    from matchmaker_amd import ops
    from matchmaker_amd.token_store import TokenStore
    dev = util.require_gpu()
    c = CR.exact_case()
    ids = [f"doc{i}" for i in range(len(c["begin"]))]
    hits = CR.token_hits_ref(c["q"], c["tokens"], c["k"])
    ref = {sr: CR.search_ref(c["q"], c["tokens"], c["begin"], c["end"], c["k"], c["top_n"], sim_round=sr, hit_rows=hits)
           for sr in (True, False)}
    src = TokenStore(torch.from_numpy(c["tokens"]).half().to(dev), ids, c["begin"], c["end"])
    f8 = src.quantize_fp8(keep_tokens=True)
    deq = ops.fp8_dequantize_rows(f8.codes, f8.scales, torch.float16)
    st16 = TokenStore(deq, ids, c["begin"], c["end"])
    return c, ids, ref, st16, f8


@pytest.mark.parametrize("use_fp16", [True, False])
def test_search_of_the_fp8_store_equals_the_restatement_and_the_16_bit_store(use_fp16):
    dev = util.require_gpu()
    c, ids, ref, st16, f8 = _exact_stores()
    assert f8.is_fp8 and torch.equal(st16.tokens, f8.tokens)               # lossless on this store
    q = torch.from_numpy(c["q"]).half().to(dev)
    s, d = f8.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16)
    assert np.array_equal(d.cpu().numpy(), ref[use_fp16][1])               # the restatement's ranking
    assert np.array_equal(s.cpu().numpy(), ref[use_fp16][0])
    s16, d16 = st16.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16)
    assert torch.equal(s, s16) and torch.equal(d, d16)                     # bit for bit
    res = f8.search(q, c["top_n"], c["k"], use_fp16=use_fp16)
    assert res == [[(ids[j], float(x)) for x, j in zip(si, di) if j >= 0] for si, di in zip(s.cpu().tolist(), d.cpu().tolist())]


def test_aggregate_of_the_fp8_store_equals_a_direct_call():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    c, ids, ref, st16, f8 = _exact_stores()
    q = torch.from_numpy(c["q"]).half().to(dev)
    cands = [[ids[j] for j in (7, 0, 199, 33)], [ids[5]], [], [ids[j] for j in range(20)], [ids[3], ids[3]]]
    out = f8.aggregate(q, cands)
    C = 20
    bb = torch.zeros(5, C, dtype=torch.int64, device=dev)
    ee = torch.zeros(5, C, dtype=torch.int64, device=dev)
    for i, l in enumerate(cands):
        for j, sid in enumerate(l):
            bb[i, j], ee[i, j] = int(c["begin"][ids.index(sid)]), int(c["end"][ids.index(sid)])
    direct = ops.maxsim_ragged_fp8(q, f8.codes, f8.scales, bb.view(-1), ee.view(-1), pairs_per_query=C, sim_round=True).view(5, C).cpu()
    assert out == [[(sid, float(direct[i, j])) for j, sid in enumerate(l)] for i, l in enumerate(cands)]
    assert out == st16.aggregate(q, cands)


def test_fp8_only_store_round_trips_and_refuses_the_token_search(tmp_path):
    from matchmaker_amd import NativeError
    from matchmaker_amd.token_store import TokenStore, write_reference_store
    dev = util.require_gpu()
    c, ids, ref, st16, f8 = _exact_stores()
    docs = [c["tokens"][b:e].astype(np.float16) for b, e in zip(c["begin"], c["end"])]
    write_reference_store(str(tmp_path / "ref"), docs, ids, token_block_size=1500, token_dtype="float16")     # three files
    only = TokenStore.load(str(tmp_path / "ref"), 128, "float16", 1500, dev, fp8=True)
    assert only.is_fp8 and torch.equal(only.codes, f8.codes) and torch.equal(only.scales, f8.scales)
    only.save_fp8(str(tmp_path / "fp8"))
    back = TokenStore.load_fp8(str(tmp_path / "fp8"), dev)
    assert torch.equal(back.codes, f8.codes) and torch.equal(back.scales, f8.scales) and back.seq_ids == ids
    q = torch.from_numpy(c["q"]).half().to(dev)
    with pytest.raises(NativeError, match="keep_tokens=True"):
        back.search_device(q, c["top_n"], c["k"])
    with pytest.raises(NativeError, match="keep_tokens=True"):
        back.tokens
    hits = f8.token_hits(q, c["k"])
    s, d = back.rank_hits(q, hits, c["top_n"])
    assert np.array_equal(d.cpu().numpy(), ref[True][1]) and np.array_equal(s.cpu().numpy(), ref[True][0])


# ------------------------------------------------------------------------------------------ graph replay
def test_ranking_the_hits_of_an_fp8_store_replays_from_a_graph_bit_equal():
    """rank_hits(trim=False) on an fp8 store captured into one graph: candidates, fp8 MaxSim, fill, selection — a single chain
    on the capturing stream, no parallel branches; the replay gives the eager result bit for bit."""
    from matchmaker_amd.token_store import TokenStore
    dev = util.require_gpu()
    rng = np.random.default_rng(22)
    lens = rng.integers(1, 71, 300)
    end = np.cumsum(lens).astype(np.int64)
    begin = end - lens
    tokens = torch.from_numpy(rng.standard_normal((int(end[-1]), 128)).astype(np.float32)).half().to(dev)
    q = torch.from_numpy(rng.standard_normal((4, 32, 128)).astype(np.float32) / np.sqrt(128)).half().to(dev)
    q[1, 20:] = 0
    st = TokenStore(tokens, list(range(300)), begin, end).quantize_fp8(keep_tokens=True)
    hits = st.token_hits(q, 32)
    s_ref, d_ref = st.rank_hits(q, hits, 40, trim=True)
    assert bool((d_ref[:, 0] >= 0).all())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                           # warm-up outside the capture
        st.rank_hits(q, hits, 40, trim=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s_g, d_g = st.rank_hits(q, hits, 40, trim=False)
    for _ in range(2):
        s_g.fill_(0)
        d_g.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_g, s_ref) and torch.equal(d_g, d_ref)
