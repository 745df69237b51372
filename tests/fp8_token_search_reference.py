"""float64 restatement of the fp8 token search (mm_dot_topk_fp8_fwd) and of the row-sharded flat search of
TokenStore.token_hits, the exact "scaled" store on which the device must reproduce it bit for bit, and the cases that
tests/test_fp8_token_search_cpu.py (preconditions, from this file alone) and tests/test_fp8_token_search_gpu.py share.

    score[q, t] = scales[t] * sum_k queries[q, k] * deq(codes[t, k])          top-k: score descending, lower row first

Scaled store: codes are integers in -8..8 written as e4m3fn bytes, scales 2^j with j in -3..3 per row, queries integers in
-2..2 — every score is a multiple of 1/8 with |score| * 8 <= 768 * 16 * 64 < 2^24, so it is exact in fp32 in any summation
order, and the values are exact in float16 and bfloat16."""
import numpy as np
import torch

from tests import dot_topk_reference as D
from tests import fp8_store_reference as F


# ---- the operators ----------------------------------------------------------------------------------------------------
def scores64(q, codes, scales):
    """[nq, N] float64"""
    return (np.asarray(q, np.float64) @ F.deq_numpy(codes).T) * np.asarray(scales, np.float64)[None, :]


def dot_topk_fp8_exact(q, codes, scales, k):
    return D.topk_of_scores(scores64(q, codes, scales), k)


def magnitudes64(q, codes, scales):
    """[nq, N] float64: scales[t] * sum_k |q_k| |deq_tk|, the sum of the magnitudes of a score's terms"""
    return (np.abs(np.asarray(q, np.float64)) @ np.abs(F.deq_numpy(codes)).T) * np.asarray(scales, np.float64)[None, :]


def score_bound(q, codes, scales):
    """[nq, N]: (E + 2) 2^-24 scales[t] sum_k |q_k| |deq_tk| — the project's (n + 2) 2^-24 sum |terms| form: E fp32 additions,
    exact products, exact scale"""
    return (np.asarray(q).shape[1] + 2) * 2.0 ** -24 * magnitudes64(q, codes, scales)


def sharded_topk_of_scores(full, k, row_shard):
    """TokenStore's row-sharded flat search on a score matrix [nq, N]: the exact top-k of every shard of row_shard consecutive
    rows (rows numbered inside the shard, -1 behind a shard shorter than k), the shard base added to the rows that exist, and a
    running [nq, k] list merged with each shard's list by mm_topk_merge's rule (running list first, input order on ties)."""
    N = full.shape[1]
    run = None
    for lo in range(0, N, row_shard):
        s, i = D.topk_of_scores(full[:, lo: lo + row_shard], k)
        i = np.where(i >= 0, i + lo, -1)
        run = (s, i) if run is None else D.topk_merge_exact(np.concatenate([run[0], s], axis=1),
                                                            np.concatenate([run[1], i], axis=1), k)
    return run


# ---- the scaled exact store -------------------------------------------------------------------------------------------
def e4m3_bytes(vals):
    """float array of e4m3fn-exact values -> uint8 codes"""
    codes = torch.from_numpy(np.asarray(vals, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(F.deq_numpy(codes), np.asarray(vals, np.float64))
    return codes


def scaled_store(nq, N, E, seed):
    """-> (queries [nq, E] float32, codes [N, E] uint8, scales [N] float32)"""
    rng = np.random.default_rng(seed)
    codes = e4m3_bytes(rng.integers(-8, 9, (N, E)))
    scales = np.ldexp(np.float32(1), rng.integers(-3, 4, N)).astype(np.float32)
    q = rng.integers(-2, 3, (nq, E)).astype(np.float32)
    return q, codes, scales


# (name, dtype, nq, N, E, k, seed).  nq 1 / 128 / 129 / 257, N 1 / 31 / 33 (one or two 32-row blocks, partial; XCDs without a
# block), 4096 / 4097 (the sampling switch; a whole and a partial last block), 20000 / 40000 / 70001 (sub-slices), every E.
CASES = [
    ("f16-1x1-e128-k1", "float16", 1, 1, 128, 1, 101),
    ("bf16-128x31-e256-k10", "bfloat16", 128, 31, 256, 10, 102),
    ("f16-129x33-e128-k100", "float16", 129, 33, 128, 100, 103),
    ("bf16-257x4096-e128-k1000", "bfloat16", 257, 4096, 128, 1000, 104),
    ("f16-257x4097-e768-k100", "float16", 257, 4097, 768, 100, 105),
    ("bf16-129x20000-e768-k1000", "bfloat16", 129, 20000, 768, 1000, 106),
    ("f16-128x70001-e128-k128", "float16", 128, 70001, 128, 128, 107),
    ("bf16-1x70001-e256-k512", "bfloat16", 1, 70001, 256, 512, 108),
    ("f16-5x40000-e128-k4096", "float16", 5, 40000, 128, 4096, 109),
    ("bf16-3x3000-e256-k4096", "bfloat16", 3, 3000, 256, 4096, 110),        # N < k
    ("f16-129x4097-e384-k100", "float16", 129, 4097, 384, 100, 111),
    ("bf16-129x4097-e512-k100", "bfloat16", 129, 4097, 512, 100, 112),
    # the switches of the fp8 kernel's launch geometry that the list above does not straddle: one query tile up to 32 queries
    # and two above; one query group up to 64 queries and two above (dim 768 too: its second tile lives in AGPRs)
    ("f16-32x33-e128-k5", "float16", 32, 33, 128, 5, 113),
    ("bf16-33x33-e128-k5", "bfloat16", 33, 33, 128, 5, 114),
    ("f16-64x100-e768-k10", "float16", 64, 100, 768, 10, 115),
    ("bf16-65x100-e768-k10", "bfloat16", 65, 100, 768, 10, 116),
    ("f16-20x4097-e768-k10", "float16", 20, 4097, 768, 10, 117),
]


# the raw-ABI case: N % 32 = 19 (a partial last block); m_scale 1e-3 / 100 / 1 gives status 1 / 2 / 0 on every row (asserted
# from the restatement by the CPU test)
RAW_ABI = ("raw-abi", "float16", 4, 59987, 128, 1000, 161)


def case_inputs(case):
    _, _, nq, N, E, _, seed = case
    return scaled_store(nq, N, E, seed)


# ---- the existing exact stores, quantised -----------------------------------------------------------------------------
def quantized(c):
    """fp8_store_reference's quantiser on a float32 corpus -> (codes, scales); `ternary` and `quarter` stores quantise
    losslessly (asserted by the CPU test)"""
    return F.quantize_numpy(c)


# ---- random data --------------------------------------------------------------------------------------------------------
RANDOM = [(dt, E, N) for dt in ("float16", "bfloat16") for E in (128, 768) for N in (5000, 70001)]


def random_inputs(dtype, E, N, nq=40, seed=7):
    """unit rows quantised by the restated quantiser, queries rounded to `dtype` -> (q float32 holding 16-bit values, codes,
    scales)"""
    rng = np.random.default_rng(seed + E + N)
    x = rng.standard_normal((N, E)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    codes, scales = F.quantize_torch(torch.from_numpy(x))
    q = rng.standard_normal((nq, E)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = torch.from_numpy(q).to(getattr(torch, dtype)).float().numpy()
    return q, codes.numpy(), scales.numpy()


def check_within_bound(full, b, k, got_s, got_i):
    """The random-data contract: returned scores within the per-score bound of float64; rows distinct, valid, in descending
    score order; no row outside the returned set beats the k-th returned float64 score by more than the two rows' bounds
    together.  full = scores64(...), b = score_bound(...) of the inputs.  Returns the worst |error| / bound."""
    nq, N = full.shape
    kk = min(k, N)
    worst = 0.0
    for r in range(nq):
        rows = got_i[r, :kk]
        assert (rows >= 0).all() and (rows < N).all() and len(set(rows.tolist())) == kk, f"row {r}: invalid or repeated rows"
        assert (got_i[r, kk:] == -1).all() and np.isneginf(got_s[r, kk:]).all()
        assert (np.diff(got_s[r, :kk]) <= 0).all(), f"row {r}: scores not descending"
        err = np.abs(got_s[r, :kk].astype(np.float64) - full[r, rows])
        assert (err <= b[r, rows]).all(), f"row {r}: score error {err.max()} above its bound"
        nz = b[r, rows] > 0
        if nz.any():
            worst = max(worst, float((err[nz] / b[r, rows][nz]).max()))
        out = np.ones(N, bool)
        out[rows] = False
        if out.any():
            j = int(np.argmin(full[r, rows]))                  # the weakest returned row, in float64
            kth, kb = full[r, rows[j]], b[r, rows[j]]
            assert (full[r, out] - b[r, out] <= kth + kb).all(), f"row {r}: a better row was left out"
    return worst
