"""numpy restatement of the quantized index (scann is not available: `import scann` fails here, as faiss does): the
anisotropic 4-bit encoder in the operation order include/mm_native.h states (float32, and a float64 twin), decode, the
scan of the codes, the exact re-score, and torch stand-ins for the operators ScannIPIndexer takes by injection.  Used by
tests/test_scann_cpu.py and tests/test_scann_gpu.py."""
import numpy as np
import torch

from tests import ivf_reference as IR


def unpack(codes):
    """codes [n, E / 4] uint8 -> [n, E / 2] block codes (the even block sits in the low nibble)"""
    codes = np.asarray(codes, np.uint8)
    out = np.empty((codes.shape[0], codes.shape[1] * 2), np.uint8)
    out[:, 0::2] = codes & 15
    out[:, 1::2] = codes >> 4
    return out


def pack(block_codes):
    b = np.asarray(block_codes, np.uint8)
    return (b[:, 0::2] | (b[:, 1::2] << 4)).astype(np.uint8)


def decode(codes, codebook):
    """-> [n, E] float64: the concatenation of every row's codewords"""
    b = unpack(codes).astype(np.int64)
    cb = np.asarray(codebook, np.float64)                          # [S, 16, 2]
    S = cb.shape[0]
    return cb[np.arange(S)[None, :], b].reshape(b.shape[0], 2 * S)


def _argmin16(cost):
    """[n, 16] -> [n]: least cost, lowest code on equal cost (what the 8, 4, 2, 1 butterfly over (cost, code) yields)"""
    return np.argmin(cost, axis=1)                                 # numpy returns the first minimum


def encode(x, lists, centroids, codebook, eta, passes, dtype=np.float32, return_gaps=False):
    """mm_ah_encode, one rounded operation of `dtype` per step in the stated order.  x [n, E], centroids [nlist, E],
    codebook [S, 16, 2]: the 16-bit values as floats.  -> codes [n, E / 4] uint8 (and, with return_gaps, [n, S] = the
    smallest relative distance between the two best costs over all decisions taken for the block)."""
    f = dtype
    x = np.asarray(x, f)
    n, E = x.shape
    S = E // 2
    lists = np.asarray(lists, np.int64)
    cent = np.asarray(centroids, f)
    ok = (lists >= 0) & (lists < cent.shape[0])
    c = np.where(ok[:, None], cent[np.where(ok, lists, 0)], f(0))
    cb = np.asarray(codebook, f)
    r = (x - c).astype(f)
    xb = x.reshape(n, S, 2)
    # |x|^2: partial c sums blocks c, c + 16, ... ascending, x0 x0 then x1 x1; then the butterfly 8, 4, 2, 1
    part = np.zeros((n, 16), f)
    for j in range(S // 16):
        blk = xb[:, 16 * j: 16 * j + 16]
        part = (part + blk[:, :, 0] * blk[:, :, 0]).astype(f)
        part = (part + blk[:, :, 1] * blk[:, :, 1]).astype(f)
    for m in (8, 4, 2, 1):
        part = (part + part[:, np.arange(16) ^ m]).astype(f)
    nrm = np.sqrt(part[:, 0]).astype(f)
    pos = nrm > 0
    inv = np.where(pos, f(1) / np.where(pos, nrm, f(1)), f(0)).astype(f)
    em1 = np.where(pos, f(np.float32(eta)) - f(1), f(0)).astype(f)
    xh = (xb * inv[:, None, None]).astype(f)
    rb = r.reshape(n, S, 2)
    cur = np.zeros((n, S), np.int64)
    gaps = np.full((n, S), np.inf)
    rows = np.arange(n)
    p = np.zeros(n, f)
    for sweep in range(passes + 1):
        for s in range(S):
            e0 = (rb[:, s, 0, None] - cb[None, s, :, 0]).astype(f)
            e1 = (rb[:, s, 1, None] - cb[None, s, :, 1]).astype(f)
            nk = ((e0 * e0).astype(f) + (e1 * e1).astype(f)).astype(f)
            tk = ((e0 * xh[:, s, 0, None]).astype(f) + (e1 * xh[:, s, 1, None]).astype(f)).astype(f)
            if sweep == 0:
                cost = nk
                po = p
            else:
                po = (p - tk[rows, cur[:, s]]).astype(f)
                u = (po[:, None] + tk).astype(f)
                cost = (nk + (em1[:, None] * (u * u).astype(f)).astype(f)).astype(f)
            best = _argmin16(cost)
            if return_gaps:
                two = np.sort(cost.astype(np.float64), axis=1)[:, :2]
                gaps[:, s] = np.minimum(gaps[:, s], (two[:, 1] - two[:, 0]) / np.maximum(np.abs(two[:, 0]), 1e-30))
            p = (po + tk[rows, best]).astype(f)
            cur[:, s] = best
    codes = pack(cur)
    return (codes, gaps) if return_gaps else codes


def loss(x, lists, centroids, codebook, codes, eta):
    """[n] float64: sum |e_s|^2 + (eta - 1) (sum <e_s, x / |x|>)^2 for the given codes (eta = 1 for an all-zero row)"""
    x = np.asarray(x, np.float64)
    lists = np.asarray(lists, np.int64)
    e = x - np.asarray(centroids, np.float64)[lists] - decode(codes, codebook)
    nrm = np.linalg.norm(x, axis=1)
    xh = x / np.maximum(nrm, 1e-300)[:, None]
    par = (e * xh).sum(axis=1)
    return (e * e).sum(axis=1) + np.where(nrm > 0, float(np.float32(eta)) - 1.0, 0.0) * par * par


def ah_scan(q, codes, codebook, list_begin, probes, probe_scores, k):
    """score = probe_scores[q, j] + <q, decode(codes[i])> over the probed union: -> (scores [nq, k] float64 descending,
    rows [nq, k] int64), (-inf, -1) padded, lower row first on equal scores"""
    q = np.asarray(q, np.float64)
    dec = decode(codes, codebook)
    lb = np.asarray(list_begin, np.int64)
    nq = q.shape[0]
    out_s = np.full((nq, k), -np.inf)
    out_r = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        rows, add = union_scores(lb, probes[i], probe_scores[i])
        if rows.size == 0:
            continue
        s = add + dec[rows] @ q[i]
        order = np.argsort(-s, kind="stable")[:k]
        out_s[i, : order.size] = s[order]
        out_r[i, : order.size] = rows[order]
    return out_s, out_r


def union_scores(list_begin, probe_row, score_row):
    """(ascending rows of the probed lists, the probe score that belongs to every one of them)"""
    parts, adds = [], []
    for l, ps in zip(probe_row, score_row):
        if l >= 0:
            rows = np.arange(list_begin[l], list_begin[l + 1], dtype=np.int64)
            parts.append(rows)
            adds.append(np.full(rows.size, float(ps)))
    if not parts:
        return np.zeros(0, np.int64), np.zeros(0)
    rows, add = np.concatenate(parts), np.concatenate(adds)
    order = np.argsort(rows, kind="stable")
    return rows[order], add[order]


def gather_dot(q, v, rows):
    """[nq, R] float64 inner products, -inf where the row is -1"""
    q, v, rows = np.asarray(q, np.float64), np.asarray(v, np.float64), np.asarray(rows, np.int64)
    out = np.einsum("qe,qre->qr", q, v[np.maximum(rows, 0)]) if v.shape[0] else np.zeros(rows.shape)
    return np.where(rows >= 0, out, -np.inf)


def search(q, centroids, codes, codebook, vectors, list_begin, nprobe, reorder, top_n):
    """the tiny indexer: probes by exact top-k over the centres, scan, re-score, stable merge -> (scores, rows)"""
    ps, probes = IR.topk_ip(q, centroids, nprobe)
    k = max(top_n, reorder)
    _, rows = ah_scan(q, codes, codebook, list_begin, probes, ps, k)
    exact = gather_dot(q, vectors, rows)
    order = np.argsort(-exact, axis=1, kind="stable")[:, :top_n]
    return np.take_along_axis(exact, order, 1), np.take_along_axis(rows, order, 1)


def exact_store(n, E, nlist, seed):
    """An encoder input on which fp32 arithmetic is exact up to the eta term: every x has 16 entries of +-1 (|x| = 4, so
    x / |x| has entries +-1/4), centres are odd multiples of 1/8 up to 3/8 (a residual never sits half-way between two
    codewords), and every block's codebook is the 4 x 4 grid {-1.5, -0.5, 0.5, 1.5}^2 in a seeded order: codewords one
    unit apart, well separated against residuals of at most 1.375.  -> (x, lists, centroids, codebook) float32 / int32"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, E), np.float32)
    for i in range(n):
        x[i, rng.permutation(E)[:16]] = rng.choice([-1.0, 1.0], 16)
    cent = (rng.choice([-3, -1, 1, 3], (nlist, E)) / 8.0).astype(np.float32)
    lists = rng.integers(0, nlist, n).astype(np.int32)
    grid = np.array([(a, b) for a in (-1.5, -0.5, 0.5, 1.5) for b in (-1.5, -0.5, 0.5, 1.5)], np.float32)
    cb = np.stack([grid[rng.permutation(16)] for _ in range(E // 2)])
    return x, lists, cent, cb


# ---- stand-ins for the injected operators (torch in, torch out) ---------------------------------------

def topk_fn(q, c, k):
    s, i = IR.topk_ip(q.float().numpy(), c.float().numpy(), k)
    return torch.from_numpy(s), torch.from_numpy(i)


def encode_fn(x, lists, centroids, codebook, eta, passes):
    return torch.from_numpy(encode(x.float().numpy(), lists.numpy(), centroids.float().numpy(), codebook.float().numpy(), eta,
                                   passes))


def scan_fn(q, codes, codebook, lb, probes, probe_scores, k):
    s, r = ah_scan(q.float().numpy(), codes.numpy(), codebook.float().numpy(), lb.numpy(), probes.numpy(),
                   probe_scores.numpy(), k)
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(r)


def rescore_fn(q, v, rows):
    return torch.from_numpy(gather_dot(q.float().numpy(), v.float().numpy(), rows.numpy()).astype(np.float32))


def merge_fn(s, ids, k):
    s = s.clone()
    s[ids < 0] = float("-inf")
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order), torch.gather(ids, 1, order)
