"""numpy restatement of the IVF inner-product index semantics (faiss is not available: oracle/np_oracle.py notes the same
for the flat index): the exact top-k over the union of the probed lists, maximum-inner-product assignment and a short
spherical k-means.  Used by tests/test_ivf_cpu.py and tests/test_ivf_gpu.py."""
import functools

import numpy as np


def ivf_scan(q, vectors, list_begin, probes, k):
    """q [nq, E], vectors [n, E] (list by list), list_begin [nlist + 1], probes [nq, nprobe] (-1 = no list).
    -> (scores [nq, k] float64 descending, rows [nq, k] int64), (-inf, -1) padded; equal scores: lower row first."""
    q = np.asarray(q, np.float64)
    v = np.asarray(vectors, np.float64)
    lb = np.asarray(list_begin, np.int64)
    nq = q.shape[0]
    out_s = np.full((nq, k), -np.inf)
    out_r = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        rows = union_rows(lb, probes[i])
        if rows.size == 0:
            continue
        s = v[rows] @ q[i]
        order = np.argsort(-s, kind="stable")[:k]          # rows ascending + stable = lower row first on ties
        out_s[i, : order.size] = s[order]
        out_r[i, : order.size] = rows[order]
    return out_s, out_r


def union_rows(list_begin, probe_row):
    """ascending rows of the lists named in one probe row"""
    lists = [int(l) for l in probe_row if l >= 0]
    assert len(set(lists)) == len(lists), "a list is probed twice"
    parts = [np.arange(list_begin[l], list_begin[l + 1], dtype=np.int64) for l in lists]
    return np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.int64)


def assign(x, centroids):
    """[n] int64: the centroid with the largest inner product (lowest number on ties)"""
    return np.argmax(np.asarray(x, np.float64) @ np.asarray(centroids, np.float64).T, axis=1).astype(np.int64)


def topk_ip(q, c, k):
    """exact inner-product top-k (scores float32, rows int64; lower row first on ties, (-inf, -1) padded)"""
    s = np.asarray(q, np.float64) @ np.asarray(c, np.float64).T
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    out_s = np.full((s.shape[0], k), -np.inf, np.float32)
    out_i = np.full((s.shape[0], k), -1, np.int64)
    out_s[:, : order.shape[1]] = np.take_along_axis(s, order, 1)
    out_i[:, : order.shape[1]] = order
    return out_s, out_i


def spherical_kmeans(x, nlist, iters=20, seed=0):
    """unit-length float16 centroids; an empty cluster takes a point of the largest one"""
    x = np.asarray(x, np.float64)
    rng = np.random.default_rng(seed)
    c = x[rng.permutation(x.shape[0])[:nlist]]
    c = (c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-20)).astype(np.float16)
    for _ in range(iters):
        a = assign(x, c)
        sums = np.zeros((nlist, x.shape[1]))
        np.add.at(sums, a, x)
        counts = np.bincount(a, minlength=nlist)
        empty = np.nonzero(counts == 0)[0]
        if empty.size:
            members = np.nonzero(a == counts.argmax())[0]
            sums[empty] = x[members[np.arange(empty.size) % members.size]]
        c = (sums / np.maximum(np.linalg.norm(sums, axis=1, keepdims=True), 1e-20)).astype(np.float16)
    return c


def clustered(n, E, n_clusters, seed, spread=0.35, dtype=np.float16):
    """a mixture of Gaussians on the unit sphere (uniform noise has no IVF structure); -> (vectors, centres)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[rng.integers(0, n_clusters, n)] + spread / np.sqrt(E) * rng.standard_normal((n, E))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(dtype), centres


# ---- two small exact problems (integer values: every fp32 sum is exact in any order, so a scan is compared bit for bit) ------
@functools.lru_cache(maxsize=None)
def carry_problem(seed=3):
    """1,030 lists over 2,000 vectors (most hold one or two rows, lists 0, 7, 500, 1023 and 1026 are empty), 1,030 queries,
    3 probes each: one element past a 1,024-wide tile in every scan over the lists and over the queries.  Query i >= 1024
    probes the non-empty list i (1027 for i = 1026), so the values behind the tile decide results.
    -> (q [1030, 128], v [2000, 128] float32 integers in -2..2, list_begin, probes [1030, 3] int32, k = 5); never modified"""
    rng = np.random.default_rng(seed)
    nlist, n, nq = 1030, 2000, 1030
    lens = np.bincount(rng.integers(0, nlist, n), minlength=nlist)
    for e in (0, 7, 500, 1023, 1026):
        lens[e + 1] += lens[e]
        lens[e] = 0
    for l in (1024, 1025, 1027, 1028, 1029):
        if lens[l] == 0:
            lens[lens.argmax()] -= 1
            lens[l] = 1
    lb = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    probes = np.stack([rng.permutation(nlist)[:3] for _ in range(nq)]).astype(np.int32)
    for i in range(1024, nq):
        own = 1027 if i == 1026 else i
        if own not in probes[i]:
            probes[i, 0] = own
    v = rng.integers(-2, 3, (n, 128)).astype(np.float32)
    q = rng.integers(-2, 3, (nq, 128)).astype(np.float32)
    return q, v, lb, probes, 5


@functools.lru_cache(maxsize=None)
def tie_problem(seed=4):
    """More ties at the k-th score than fit: lists of 30, 50, 0, 20 and 60 rows, both queries probe lists 1 and 4 around a
    hole.  40 bit-identical rows (20 in each probed list, scattered) score 0 for query 0, seven rows score 1 .. 7 and the
    other probed rows -6 .. -1: with k = 10 the tie group starts at rank 8 and three of its 40 rows fit.
    -> (q [2, 128], v [160, 128] float32 integers in -6..7, list_begin, probes [2, 3] int32, k = 10, the group's rows ascending)"""
    rng = np.random.default_rng(seed)
    lens = [30, 50, 0, 20, 60]
    lb = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(lb[-1])
    q = rng.integers(-2, 3, (2, 128)).astype(np.float32)
    q[0, 0] = 1
    q[0, 64:] = 0                                  # query 0 sees element 0 of a probed row (elements 1 .. 63 are zero there)
    v = rng.integers(-2, 3, (n, 128)).astype(np.float32)
    probed = np.concatenate([np.arange(lb[1], lb[2]), np.arange(lb[4], lb[5])])
    group = np.sort(np.concatenate([rng.permutation(np.arange(lb[1], lb[2]))[:20], rng.permutation(np.arange(lb[4], lb[5]))[:20]]))
    others = rng.permutation(np.setdiff1d(probed, group))
    v[probed, :64] = 0
    v[group] = v[group[0]]                         # bit-identical rows
    v[others[:7], 0] = np.arange(1, 8)
    v[others[7:], 0] = -rng.integers(1, 7, others.size - 7)
    probes = np.array([[4, -1, 1], [1, 4, -1]], np.int32)
    return q, v, lb, probes, 10, group
