"""numpy (float64) restatement of the k-means operators and of the dynamic IVF index (mm_kmeans_assign,
mm_kmeans_segment_sum, matchmaker_amd.retrieval.DynamicIVFIndexer), plus the stand-ins that run the host logic without a
device.  Used by tests/test_kmeans_cpu.py and tests/test_kmeans_gpu.py; the scan semantics come from tests/ivf_reference.py."""
import numpy as np
import torch

from tests import ivf_reference as IR


def exact_store(n, E, seed, dtype=np.float32):
    """multiples of 1/4 in [-2, 2]: every product is a multiple of 1/16 below 4 and every partial sum is exact in fp32 in
    any order (E <= 768: |sum| <= 3072 = 49152 / 16 < 2^24 / 16), and the values are exact in float16 and bfloat16"""
    return (np.random.default_rng(seed).integers(-8, 9, (n, E)) / 4.0).astype(dtype)


def assign(x, centroids):
    """-> (list [n] int64: the centroid of maximum inner product, lowest number on ties; score [n] float64)"""
    s = np.asarray(x, np.float64) @ np.asarray(centroids, np.float64).T
    a = np.argmax(s, axis=1).astype(np.int64)
    return a, s[np.arange(s.shape[0]), a] if s.shape[0] else np.zeros(0)


def margin_and_bound(x, centroids):
    """per row: (best - second best score, sum_i |x_i c_i| maximised over the centroids, the float64 score matrix)"""
    x = np.asarray(x, np.float64)
    c = np.asarray(centroids, np.float64)
    s = x @ c.T
    top = np.sort(s, axis=1)
    margin = top[:, -1] - top[:, -2] if c.shape[0] > 1 else np.full(x.shape[0], np.inf)
    return margin, (np.abs(x) @ np.abs(c).T).max(axis=1), s


def lists_of(a, nlist):
    """assignment -> (order: rows list by list, input order inside a list; list_begin [nlist + 1])"""
    order = np.argsort(a, kind="stable").astype(np.int64)
    lb = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    return order, lb


def segment_sum(x, order, list_begin):
    """sums [nlist, E] float64; rows of `order` outside [0, n) are skipped"""
    x = np.asarray(x, np.float64)
    lb = np.asarray(list_begin, np.int64)
    out = np.zeros((lb.shape[0] - 1, x.shape[1]))
    for l in range(lb.shape[0] - 1):
        rows = np.asarray(order[lb[l]: lb[l + 1]], np.int64)
        rows = rows[(rows >= 0) & (rows < x.shape[0])]
        out[l] = x[rows].sum(axis=0)
    return out


def segment_abs_sum(x, order, list_begin):
    return segment_sum(np.abs(np.asarray(x, np.float64)), order, list_begin)


# ---- stand-ins for the device operators (torch CPU tensors in and out) ------------------------------------------------

def assign_fn(x, centroids):
    a, s = assign(x.float().numpy(), centroids.float().numpy())
    return torch.from_numpy(a.astype(np.int32)), torch.from_numpy(s.astype(np.float32))


def sum_fn(x, order, list_begin):
    """fp32, rows added one after the other in list order: what index_add_ over the rows in input order gives on the CPU"""
    lb = list_begin.numpy()
    nlist = lb.shape[0] - 1
    sums = np.zeros((nlist, x.shape[1]), np.float32)
    np.add.at(sums, np.repeat(np.arange(nlist), np.diff(lb)), x.float().numpy()[order.numpy()[lb[0]: lb[-1]]])
    return torch.from_numpy(sums)


def scan_fn(q, v, lb, probes, k):
    s, r = IR.ivf_scan(q.float().numpy(), v.float().numpy(), lb.numpy(), probes.numpy(), k)
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(r)


class ListModel:
    """the dynamic index as plain Python: per list the (id, vector) entries in arrival order; an update removes every entry
    with one of the ids, then appends the new ones"""

    def __init__(self, centroids):
        self.centroids = np.asarray(centroids, np.float64)
        self.lists = [[] for _ in range(self.centroids.shape[0])]

    def add(self, ids, vecs):
        a, _ = assign(vecs, self.centroids)
        for i, l, v in zip(ids, a, vecs):
            self.lists[int(l)].append((int(i), np.asarray(v, np.float64)))

    def update(self, ids, vecs):
        gone = set(int(i) for i in ids)
        self.lists = [[e for e in lst if e[0] not in gone] for lst in self.lists]
        self.add(ids, vecs[: len(ids)])

    def ids_of(self, l):
        return [e[0] for e in self.lists[l]]

    def layout(self):
        """-> (vectors list by list, ids, list_begin) as the index's scan sees them"""
        E = self.centroids.shape[1]
        vec = np.array([e[1] for lst in self.lists for e in lst]).reshape(-1, E)
        ids = np.array([e[0] for lst in self.lists for e in lst], np.int64)
        lb = np.concatenate([[0], np.cumsum([len(lst) for lst in self.lists])]).astype(np.int64)
        return vec, ids, lb

    def search_single(self, q, top_n):
        """-> (scores float64, ids, centroid ids [nq, 1]): the exact top_n of the one probed list"""
        q = np.atleast_2d(np.asarray(q, np.float64))
        c, _ = assign(q, self.centroids)
        vec, ids, lb = self.layout()
        s, rows = IR.ivf_scan(q, vec, lb, c[:, None], top_n)
        return s, np.where(rows >= 0, ids[np.maximum(rows, 0)] if ids.size else rows, -1), c[:, None]
