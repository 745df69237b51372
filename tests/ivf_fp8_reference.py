"""float64 restatement of the fp8 IVF list scan (mm_ivf_scan_fp8_fwd) and the inputs that
tests/test_ivf_fp8_cpu.py (preconditions, from this file alone) and tests/test_ivf_fp8_gpu.py share.

    score(q, t) = scales[t] * sum_k queries[q, k] * deq(codes[t, k])    for every row t of the lists in probes[q, :]
    top-k over that union: score descending, lower row first (union ascending + stable sort), (-inf, -1) padded

The restatement is tests/ivf_reference.py's scan over tests/fp8_token_search_reference.py's score values.  The exact store
is that module's `scaled_store` (integer codes in -8..8, scales 2^-3..2^3 per row, integer queries in -2..2), laid out over
the lists of tests/test_ivf_gpu.py with probes drawn as its `_problem` draws them."""
import numpy as np
import torch

from tests import fp8_store_reference as F
from tests import fp8_token_search_reference as R
from tests import ivf_reference as IR

# tests/test_ivf_gpu.py's lists: empty lists, one and two blocks, partial last blocks of 1 / 15 / 17 / 31 / 33 rows
LENS = [0, 1, 15, 16, 17, 3000, 0, 33, 5000, 64, 2500, 100, 31, 32, 4097]
NLIST = len(LENS)
N_ROWS = sum(LENS)                                           # 14,906


def list_begin():
    return np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)


def ivf_scan_fp8(q, codes, scales, lb, probes, k, full=None):
    """-> (scores [nq, k] float64 descending, rows [nq, k] int64), (-inf, -1) padded; equal scores: lower row first.
    full: scores64(q, codes, scales) when the caller already has it."""
    q = np.asarray(q, np.float64)
    nq = q.shape[0]
    out_s = np.full((nq, k), -np.inf)
    out_r = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        rows = IR.union_rows(lb, probes[i])
        if rows.size == 0:
            continue
        s = full[i, rows] if full is not None else R.scores64(q[i: i + 1], codes[rows], scales[rows])[0]
        order = np.argsort(-s, kind="stable")[:k]           # rows ascending + stable = lower row first on ties
        out_s[i, : order.size] = s[order]
        out_r[i, : order.size] = rows[order]
    return out_s, out_r


def draw_probes(nq, nprobe, seed, nlist=NLIST):
    """tests/test_ivf_gpu.py's probes: a seeded permutation per query; query 0 probes lists 8, 5 and 3 around holes"""
    probes = np.stack([np.random.default_rng(seed + i).permutation(nlist)[:nprobe] for i in range(nq)]).astype(np.int32)
    probes[0, :4] = [8, -1, 5, 3]                            # (nprobe >= 4)
    probes[0, 4:] = -1
    return probes


def exact_problem(E, nq, nprobe, seed):
    """-> (q [nq, E] float32, codes [N_ROWS, E] uint8, scales [N_ROWS] float32, list_begin, probes) on the scaled store"""
    q, codes, scales = R.scaled_store(nq, N_ROWS, E, seed)
    return q, codes, scales, list_begin(), draw_probes(nq, nprobe, seed)


# the exact cases of the GPU suite: (E, nq, k), nprobe 6, both query dtypes
EXACT = [(128, 1, 1), (128, 37, 10), (128, 700, 1000), (256, 37, 10), (384, 1, 1000), (384, 700, 10), (512, 37, 1),
         (768, 1, 10), (768, 37, 1000), (768, 700, 1),
         (128, 3, 16), (128, 3, 4096)]         # k equal to its padded power of two; the operator's limit
EXACT_NPROBE = 6


def exact_seed(E, nq, k):
    return E + nq + k


def short_union_probes():
    """the five queries of test_ivf_scan_k_larger_than_the_union_and_empty_rows: 16, 0, 17, 31 and 0 candidates"""
    probes = np.full((5, 4), -1, np.int32)
    probes[0, :2] = [1, 2]            # 1 + 15 rows
    probes[1, 0] = 0                  # an empty list only
    probes[2, :3] = [6, 0, 4]         # empty, empty, 17
    probes[3, 2] = 12                 # 31, behind two holes
    return probes                     # query 4 probes nothing at all


SHORT_FOUND = [16, 0, 17, 31, 0]


def tie_problem():
    """tests/ivf_reference.py's tie problem with its rows quantised (integers up to 7: exact in e4m3fn under a power-of-two
    scale) -> (q, codes [n, 128] uint8, scales [n] float32, list_begin, probes, k, the tie group's rows ascending)"""
    q, v, lb, probes, k, group = IR.tie_problem()
    codes, scales = F.quantize_torch(torch.from_numpy(v).half())
    return q, codes.numpy(), scales.numpy(), lb, probes, k, group


# ---- random unit rows -----------------------------------------------------------------------------------------------------
def random_problem(dtype, E, nq=40, nprobe=6, seed=7):
    """unit rows over LENS quantised by the restated quantiser, unit queries rounded to `dtype`, probes as above"""
    q, codes, scales = R.random_inputs(dtype, E, N_ROWS, nq=nq, seed=seed)
    return q, codes, scales, list_begin(), draw_probes(nq, nprobe, seed + E)


def check_union_within_bound(q, codes, scales, lb, probes, k, got_s, got_r):
    """fp8_token_search_reference.check_within_bound per query, on the columns of the probed union: scores within
    (E + 2) 2^-24 scales[t] sum_k |q_k| |deq_tk| of float64 (E fp32 additions plus the final add; exact products, exact
    scale); rows distinct, inside the union, descending; nothing left out beats the k-th by more than the two bounds together;
    (-inf, -1) behind a short union.  Returns the worst |error| / bound."""
    worst = 0.0
    for r in range(np.asarray(q).shape[0]):
        union = IR.union_rows(lb, probes[r])
        if union.size == 0:
            assert (got_r[r] == -1).all() and np.isneginf(got_s[r]).all(), f"query {r}: an empty union returned rows"
            continue
        full = R.scores64(q[r: r + 1], codes[union], scales[union])
        b = R.score_bound(q[r: r + 1], codes[union], scales[union])
        rows = got_r[r]
        live = rows >= 0
        assert np.isin(rows[live], union).all(), f"query {r}: a row outside the probed lists"
        pos = np.where(live, np.searchsorted(union, np.where(live, rows, union[0])), -1)
        worst = max(worst, R.check_within_bound(full, b, k, got_s[r: r + 1], pos[None, :]))
    return worst


# ---- the random-normal ColBERT store of the end-to-end test ------------------------------------------------------------------
NORMAL_SEED = 22                                             # clear at the cut (test_ivf_fp8_cpu.py); 21, 23, 24 are not
NORMAL_K = 16


def normal_store(seed=NORMAL_SEED, n_docs=200):
    """200 documents of 1..70 rows, rows standard_normal -> fp16, 4 x 32 query tokens / sqrt(128) -> fp16 with q[1, 20:] = 0
    (the generator of tests/test_colbert_search_gpu.py) -> (tokens [T, 128] fp16 tensor, q [4, 32, 128] fp16 tensor, begin, end)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 71, n_docs)
    end = np.cumsum(lens).astype(np.int64)
    begin = end - lens
    tokens = torch.from_numpy(rng.standard_normal((int(end[-1]), 128)).astype(np.float32)).half()
    q = torch.from_numpy(rng.standard_normal((4, 32, 128)).astype(np.float32) / np.sqrt(128)).half()
    q[1, 20:] = 0
    return tokens, q, begin, end


def normal_store_gap_over_bound(seed=NORMAL_SEED, k=NORMAL_K):
    """Over the live query tokens: the smallest of (score_k - score_{k+1}) / (bound_k + bound_{k+1}) in float64 on the
    quantised store, and the smallest gap over 2 x the largest bound of the token (the conservative form)."""
    tokens, q, _, _ = normal_store(seed)
    codes, scales = F.quantize_torch(tokens)
    qq = q.reshape(-1, 128).float().numpy()
    qq = qq[(qq != 0).any(axis=1)]
    full = R.scores64(qq, codes.numpy(), scales.numpy())
    b = R.score_bound(qq, codes.numpy(), scales.numpy())
    order = np.argsort(-full, axis=1, kind="stable")[:, : k + 1]
    s = np.take_along_axis(full, order, 1)
    bb = np.take_along_axis(b, order, 1)
    gap = s[:, k - 1] - s[:, k]
    return float((gap / (bb[:, k - 1] + bb[:, k])).min()), float((gap / (2 * b.max(axis=1))).min())
