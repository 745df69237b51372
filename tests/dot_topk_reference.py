"""numpy (float64) restatement of mm_dot_topk_fwd and mm_topk_merge with their tie rules built in, the exact-valued stores
on which the device must reproduce it bit for bit, and the cases that tests/test_dot_topk_reference_cpu.py (preconditions,
from this file alone) and tests/test_dot_topk_exact_gpu.py (the device) share.

Exact stores: every inner product is an integer (ternary) or a multiple of 1/16 (kmeans_reference.exact_store) far below
2^24 units, so it is exact in fp32 in ANY summation order, and the values are exact in float16 and bfloat16.  The device
result then has to EQUAL the float64 one: scores, rows, and the order inside every tie group."""
import functools

import numpy as np

from tests.kmeans_reference import exact_store

K_MAX = 4096          # include/mm_native.h: k <= 4096
SEL_MAX = 1024        # csrc/dot_topk.hip kSelMax: more entries than this at or above the k-th score -> the full-sort path
SAMPLE = 16384        # csrc/dot_topk.hip kDotSample
MERGE_MAX = 16384     # include/mm_native.h: n_in <= 16384


# ---- the operators ----------------------------------------------------------------------------------------------------

def scores64(q, c):
    return np.asarray(q, np.float64) @ np.asarray(c, np.float64).T


def topk_of_scores(full, k):
    """[nq, N] float64 -> (scores [nq, k] float64, rows [nq, k] int64): score descending, lower row first on ties (a stable
    argsort of the negated scores), (-inf, -1) behind the N-th entry"""
    nq, N = full.shape
    order = np.argsort(-full, axis=1, kind="stable")[:, :k]
    s = np.full((nq, k), -np.inf)
    i = np.full((nq, k), -1, np.int64)
    s[:, : order.shape[1]] = np.take_along_axis(full, order, axis=1)
    i[:, : order.shape[1]] = order
    return s, i


def dot_topk_exact(q, c, k):
    return topk_of_scores(scores64(q, c), k)


def topk_merge_exact(scores, ids, k):
    """rows of (score, id) -> the k best per row: entries with id < 0 dropped whatever their score, the rest by score
    descending, input order on ties; (-inf, -1) behind them"""
    scores = np.asarray(scores, np.float64)
    ids = np.asarray(ids, np.int64)
    nq = scores.shape[0]
    out_s = np.full((nq, k), -np.inf)
    out_i = np.full((nq, k), -1, np.int64)
    for r in range(nq):
        keep = np.nonzero(ids[r] >= 0)[0]
        keep = keep[np.argsort(-scores[r, keep], kind="stable")][:k]
        out_s[r, : keep.size] = scores[r, keep]
        out_i[r, : keep.size] = ids[r, keep]
    return out_s, out_i


def tie_stats(full, k):
    """per row of the score matrix: (documents at or above the k-th score, documents AT the k-th score); k > N: the N-th"""
    full = np.asarray(full, np.float64)
    N = full.shape[1]
    kk = min(k, N)
    kth = -np.partition(-full, kk - 1, axis=1)[:, kk - 1]
    return (full >= kth[:, None]).sum(axis=1), (full == kth[:, None]).sum(axis=1)


# ---- what the native call documents about itself ----------------------------------------------------------------------

def pow2_ge(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def cap_of(N, k):
    """candidate slots per query (csrc/dot_topk.hip dot_cap): a row converges only if the documents at or above its k-th
    score fit"""
    c = max(1024, pow2_ge(4 * k))
    return max(c, 4096) if N <= 4096 else c


def sampled_survivors(full, k, m_scale):
    """Documents the FIRST native call files per row: those at or above the m-th largest score of the strided sample
    (every (N // S)-th document, S = min(N, 16384); m = 2.5 k m_scale S / N rounded, in [4, S]); every document when
    N <= 4096.  status = 1 when fewer than min(k, N), 2 when more than cap_of(N, k)."""
    full = np.asarray(full, np.float64)
    N = full.shape[1]
    if N <= 4096:
        return np.full(full.shape[0], N)
    S = min(N, SAMPLE)
    sample = full[:, : S * (N // S): N // S]
    m = min(max(int(2.5 * k * float(np.float32(m_scale)) * S / N + 0.5), 4), S)
    tau = -np.partition(-sample, m - 1, axis=1)[:, m - 1]
    return (full >= tau[:, None]).sum(axis=1)


# ---- stores -----------------------------------------------------------------------------------------------------------

def ternary_store(n, E, seed, dtype=np.float32):
    """entries in {-1, 0, 1}: integer scores, |s| <= E <= 768; ties at the k-th rank run to hundreds"""
    return np.random.default_rng(seed).integers(-1, 2, (n, E)).astype(dtype)


def store(kind, n, E, seed):
    if kind == "ternary":
        return ternary_store(n, E, seed)
    if kind == "quarter":
        return exact_store(n, E, seed)
    raise ValueError(kind)


def inputs(kind, nq, N, E, seed):
    """-> (queries [nq, E], corpus [N, E]) float32.  kind "nonpos": queries |ternary|, corpus -|ternary| (every score <= 0)"""
    if kind == "nonpos":
        return np.abs(ternary_store(nq, E, seed + 1)), -np.abs(ternary_store(N, E, seed))
    return store(kind, nq, E, seed + 1), store(kind, N, E, seed)


def planted(nq, N, E, rows, seed):
    """a ternary corpus in which the documents `rows` are copies of query 0, which has no zero entry: they score E against
    it, every other document less.  -> (queries, corpus)"""
    q, c = inputs("ternary", nq, N, E, seed)
    q[0] = np.where(q[0] == 0, 1.0, q[0])
    c[np.asarray(rows)] = q[0]
    return q, c


def scattered_rows(N, n, seed):
    """n distinct rows of [0, N), ascending, not a regular pattern"""
    return np.sort(np.random.default_rng(seed).permutation(N)[:n])


# ---- shared cases -----------------------------------------------------------------------------------------------------
# (name, store, dtype, nq, N, E, k, seed): the instantiation sweep.  Every E in each dtype; nq 1 / 128 / 129 / 257 = one and
# two query tiles with partial groups; N 1 / 31 / 33 (one or two blocks, partial), 4096 / 4097 (the sampling switch), 20000,
# 70001 (sub-slices, partial last block); E = 768 with nq > 128 is the two-accumulator-set form.
SWEEP = [
    ("f16-t-1x1-e128-k1", "ternary", "float16", 1, 1, 128, 1, 11),
    ("bf16-q-128x31-e256-k10", "quarter", "bfloat16", 128, 31, 256, 10, 12),
    ("f16-q-129x33-e384-k100", "quarter", "float16", 129, 33, 384, 100, 13),
    ("bf16-t-257x4096-e512-k1000", "ternary", "bfloat16", 257, 4096, 512, 1000, 14),
    ("f16-t-257x4097-e768-k100", "ternary", "float16", 257, 4097, 768, 100, 15),
    ("bf16-t-129x20000-e768-k1000", "ternary", "bfloat16", 129, 20000, 768, 1000, 16),
    ("f16-q-128x70001-e128-k10", "quarter", "float16", 128, 70001, 128, 10, 17),
    ("bf16-t-1x70001-e256-k100", "ternary", "bfloat16", 1, 70001, 256, 100, 18),
    ("f16-t-257x20000-e512-k1", "ternary", "float16", 257, 20000, 512, 1, 19),
    ("bf16-q-129x4097-e384-k1000", "quarter", "bfloat16", 129, 4097, 384, 1000, 20),
    ("f16-q-1x4096-e256-k10", "quarter", "float16", 1, 4096, 256, 10, 21),
    ("bf16-t-128x33-e128-k1", "ternary", "bfloat16", 128, 33, 128, 1, 22),
    ("bf16-q-129x70001-e768-k100", "quarter", "bfloat16", 129, 70001, 768, 100, 23),
    ("f16-t-128x20000-e384-k100", "ternary", "float16", 128, 20000, 384, 100, 24),
]

# k > 1024: the full bitonic sort over cap = 8192 / 16384 entries; the last one is a shard smaller than k
LARGE_K = [
    ("k1025", "ternary", "float16", 3, 40000, 256, 1025, 31),
    ("k2000", "ternary", "bfloat16", 3, 40000, 256, 2000, 32),
    ("k4096", "ternary", "float16", 3, 40000, 256, 4096, 33),
    ("k4096-n3000", "ternary", "float16", 3, 3000, 256, 4096, 34),
]

# every score <= 0: a phantom zero (an idle accumulator, a padded slot) would rank first
NEGATIVE = [
    ("neg-200x31-e768", "nonpos", "float16", 200, 31, 768, 5, 41),
    ("neg-200x40-e768", "nonpos", "float16", 200, 40, 768, 10, 42),
    ("neg-200x5000-e768", "nonpos", "float16", 200, 5000, 768, 100, 43),
    ("neg-5x5000-e128", "nonpos", "bfloat16", 5, 5000, 128, 100, 44),
]

# more than 32 query groups of 256: the launch loop's second iteration serves queries 8192 ..
MANY_GROUPS = ("groups33", "quarter", "float16", 8200, 4500, 128, 10, 51)

# both sort paths of the row kernel in one call: rows with more and with fewer than 1,024 entries at or above the k-th score
MIXED_TIES = ("mixed-ties", "ternary", "float16", 16, 20000, 128, 1000, 3)

RAW_ABI = ("raw-abi", "quarter", "float16", 4, 60000, 128, 1000, 61)


def case_inputs(case):
    _, kind, _, nq, N, E, _, seed = case
    return inputs(kind, nq, N, E, seed)


def mixed_ties_inputs():
    """seed-3 numpy ternary store, N = 20000, E = 128, 16 queries"""
    rng = np.random.default_rng(3)
    c = rng.integers(-1, 2, (20000, 128)).astype(np.float32)
    q = rng.integers(-1, 2, (16, 128)).astype(np.float32)
    return q, c


def planted_1500():
    """1,500 identical best documents on scattered rows, k = 1000, cap = 4096 -> (q, c, rows, k)"""
    rows = scattered_rows(20000, 1500, 71)
    q, c = planted(3, 20000, 128, rows, 72)
    return q, c, rows, 1000


def planted_5000():
    """5,000 identical best documents, k = 1000, cap = 4096: more ties than candidate slots -> (q, c, rows, k)"""
    rows = scattered_rows(20000, 5000, 73)
    q, c = planted(2, 20000, 128, rows, 74)
    return q, c, rows, 1000


def planted_sampled_1100():
    """1,100 identical best documents on the first 1,100 rows the strided sample visits (N = 70001: every 4th row), k = 400:
    the sample's m = 234th largest is the group's score on each of the 1,024 per-thread maxima, more than 1,024 sample keys
    reach it (the tie-heavy fall-through of the threshold select), and the row kernel meets 1,100 > 1,024 entries at the
    k-th score.  cap = 2048 -> (q, c, rows, k)"""
    rows = 4 * np.arange(1100)
    q, c = planted(2, 70001, 128, rows, 75)
    return q, c, rows, 400


def merge_inputs(n_in, seed=81):
    """-> (scores [3, n_in] float32, ids [3, n_in] int64).  Row 0: integer scores from 8 values, ids above 2^40, every
    seventh position (from the second) padding that carries +1e30.  Row 1: padding only, with finite and infinite scores.
    Row 2: as row 0 with other padding positions, and the valid entry in the middle scores -inf."""
    rng = np.random.default_rng(seed + n_in)
    s = rng.integers(0, 8, (3, n_in)).astype(np.float32)
    ids = (1 << 40) + np.stack([rng.permutation(n_in) for _ in range(3)]).astype(np.int64) * 3
    ids[0, 1::7] = -1
    s[0, 1::7] = 1e30
    ids[1] = -1
    s[1, ::2] = 1e30
    s[1, 1::3] = np.inf
    ids[2, 3::5] = -1
    s[2, 3::5] = 1e30
    ids[2, n_in // 2] = (1 << 41) + 5
    s[2, n_in // 2] = -np.inf
    return s, ids


SHARDS = (9000, 7000, 3950, 50)


@functools.lru_cache(maxsize=2)
def shard_inputs():
    return inputs("ternary", 9, sum(SHARDS), 128, 91)
