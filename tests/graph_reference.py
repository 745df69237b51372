"""numpy (float64) restatement of the graph index: the exact construction of matchmaker_amd.retrieval.GraphIPIndexer and the
beam search of mm_graph_search_fwd, plus the stand-ins that run the indexer's host logic without a device.  Used by
tests/test_graph_cpu.py and tests/test_graph_gpu.py."""
import numpy as np
import torch

from tests.kmeans_reference import exact_store  # noqa: F401  (the stores of the bit-equal tests)


def topk_ip(q, c, k):
    """exact inner-product top-k, score descending, lower row first on ties; (-inf, -1) padded when c has fewer than k rows"""
    s = np.asarray(q, np.float64) @ np.asarray(c, np.float64).T
    nq, n = s.shape
    out_s = np.full((nq, k), -np.inf)
    out_i = np.full((nq, k), -1, np.int64)
    kk = min(k, n)
    for r in range(nq):
        order = np.lexsort((np.arange(n), -s[r]))[:kk]
        out_s[r, :kk] = s[r, order]
        out_i[r, :kk] = order
    return out_s, out_i


def knn_lists(x, M):
    """[N, M] int64: the M rows of highest inner product with every row, without the row itself (-1 padded when N - 1 < M):
    the top M + 1, the row itself dropped when present, else the last entry"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    _, idx = topk_ip(x, x, M + 1)
    knn = np.full((n, M), -1, np.int64)
    for v in range(n):
        row = idx[v].tolist()
        if v in row:
            row.remove(v)
        else:
            row.pop()
        knn[v] = row
    return knn


def build(x, M):
    """neighbors [N, M] int32, -1 padded: forward edges knn[v][:M/2], then the reverse edges u (u -> v a forward edge) by
    (rank of v in fwd[u], u), then knn[v][M/2:]; no entry twice, at most M"""
    assert M % 2 == 0 and 2 <= M <= 128
    knn = knn_lists(x, M)
    n, H = knn.shape[0], M // 2
    fwd = knn[:, :H]
    rev = [[] for _ in range(n)]
    for r in range(H):
        for u in range(n):
            v = fwd[u, r]
            if v >= 0:
                rev[v].append(u)
    g = np.full((n, M), -1, np.int32)
    for v in range(n):
        row = [int(t) for t in fwd[v] if t >= 0]
        have = set(row)
        for u in rev[v] + [int(t) for t in knn[v, H:] if t >= 0]:
            if len(row) == M:
                break
            if u not in have:
                have.add(u)
                row.append(u)
        g[v, : len(row)] = row
    return g


def search(x, g, q, entry_rows, ef, width, max_iters, k):
    """-> (scores [nq, k] float64, rows [nq, k] int64, iters [nq], scored [nq])"""
    x = np.asarray(x, np.float64)
    q = np.atleast_2d(np.asarray(q, np.float64))
    entry_rows = np.asarray(entry_rows).reshape(q.shape[0], -1)
    nq = q.shape[0]
    out_s = np.full((nq, k), -np.inf)
    out_r = np.full((nq, k), -1, np.int64)
    iters = np.zeros(nq, np.int64)
    scored = np.zeros(nq, np.int64)
    for qi in range(nq):
        visited, expanded = set(), set()
        new = []
        for r in entry_rows[qi].tolist():
            if r >= 0 and r not in visited:
                visited.add(r)
                new.append(r)
        L = []

        def merge(rows):
            nonlocal L
            if rows:
                s = x[rows] @ q[qi]
                L = sorted(L + [(-float(a), int(b)) for a, b in zip(s, rows)])[:ef]
            scored[qi] += len(rows)

        merge(new)
        for _ in range(max_iters):
            pick = [r for _, r in L if r not in expanded][:width]
            if not pick:
                break
            iters[qi] += 1
            expanded.update(pick)
            new = []
            for r in pick:
                for nb in g[r].tolist():
                    if nb >= 0 and nb not in visited:
                        visited.add(nb)
                        new.append(nb)
            merge(new)
        kk = min(k, len(L))
        out_s[qi, :kk] = [-a for a, _ in L[:kk]]
        out_r[qi, :kk] = [b for _, b in L[:kk]]
    return out_s, out_r, iters, scored


def default_max_iters(ef, width):
    return -(-ef // width) + 8


def recall_collection(n=4096, E=128, nq=64, centres=16, seed=7):
    """16 unit-norm Gaussian centres; rows and queries = a random centre + N(0, I / E) noise, rounded to fp16
    -> (x [n, E] float16, q [nq, E] float16)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, E))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, centres, n)] + rng.standard_normal((n, E)) / np.sqrt(E)
    q = c[rng.integers(0, centres, nq)] + rng.standard_normal((nq, E)) / np.sqrt(E)
    return x.astype(np.float16), q.astype(np.float16)


def sample_rows(n, S):
    """the entry sample: rows floor(i n / S), i < S = min(n, S)"""
    S = min(n, S)
    return (np.arange(S, dtype=np.int64) * n) // S


def entries_from_sample(x, q, sample, count):
    """entry_rows [nq, count] int32: the `count` rows of the sample with the highest inner product"""
    _, i = topk_ip(q, np.asarray(x, np.float64)[sample], count)
    return np.where(i >= 0, sample[np.maximum(i, 0)], -1).astype(np.int32)


def recall_at(rows, truth, k):
    return float(np.mean([len(set(rows[r, :k].tolist()) & set(truth[r, :k].tolist())) / k for r in range(rows.shape[0])]))


# ---- stand-ins for the device operators (torch CPU tensors in and out) ------------------------------------------------

def topk_fn(q, c, k):
    s, i = topk_ip(q.float().numpy(), c.float().numpy(), k)
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(i)


def search_fn(q, v, g, entry_rows, ef, k, width=4, max_iters=None):
    mi = default_max_iters(ef, width) if max_iters is None else max_iters
    s, r, _, _ = search(v.float().numpy(), g.numpy(), q.float().numpy(), entry_rows.numpy(), ef, width, mi, k)
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(r)


def merge_fn(s, ids, k):
    s = s.clone()
    s[ids < 0] = float("-inf")
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order), torch.gather(ids, 1, order)
