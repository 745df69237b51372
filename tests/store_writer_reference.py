"""Restatement of the host half of the reference's encode loop (matchmaker/dense_retrieval.py:237-265) over a sequence of
batches, in numpy: which rows a document keeps (:244 `current_reps[np.abs(current_reps).sum(-1) > 0, :]`, in the output's own
dtype), the rows back to back (:259-261), the row range of every document (:264) and the per-file layout (:248-256).

bfloat16 has no numpy dtype: its rows travel as int16 bit patterns and the row test runs on their exact float32 values (a sum
of non-negative values is zero only if every one is, in either type).  `append_standin` is a torch-CPU function with
ops.store_append's signature that obeys the C ABI's semantics (include/mm_native.h) — the bit test of the magnitudes, the
all-or-nothing capacity rule, the sticky status — for the CPU suite to drive TokenStoreWriter with.
"""
import numpy as np
import torch

from tests import fp8_store_reference as R8

_BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bit patterns of a float tensor (bit equality, NaN-proof and -0.0-aware)."""
    return t.view(_BITS[t.dtype])


def keep_mask(x: torch.Tensor) -> np.ndarray:
    """[B, D] bool: :244 for every document of x [B, D, E] (CPU) — one reduction over the last axis, which is what the
    per-document statement computes for each of them."""
    a = x.float().numpy() if x.dtype == torch.bfloat16 else x.numpy()
    return np.abs(a).sum(-1) > 0


def append_batches(batches, fill0: int = 0):
    """batches: [(x [B, D, E] CPU tensor, keep_all)] in append order.  Returns (rows [T, E] of x's dtype = the kept rows back
    to back in document order, then token order; begin [n] int64; end [n] int64) with the ranges counted from fill0."""
    rows, begin, end = [], [], []
    at = fill0
    for x, keep_all in batches:
        keep = np.ones(x.shape[:2], dtype=bool) if keep_all else keep_mask(x)
        rows.append(x[torch.from_numpy(keep)])                             # row-major: document by document
        e = at + np.cumsum(keep.sum(1), dtype=np.int64)
        begin.append(e - keep.sum(1))
        end.append(e)
        at = int(e[-1]) if e.size else at
    return torch.cat(rows), np.concatenate(begin).astype(np.int64), np.concatenate(end).astype(np.int64)


def file_layout(lens, token_block_size: int):
    """:248-264 for documents of `lens` rows: ([(file, start, end)] per document, storage_filled_to_index)."""
    infos, filled = [], []
    n, ins = 0, 0
    for k in lens:
        k = int(k)
        if ins + k > token_block_size:
            filled.append(ins)
            n, ins = n + 1, 0
        infos.append((n, ins, ins + k))
        ins += k
    filled.append(ins)
    return infos, filled


def append_standin(x, rows_out, codes_out, scales_out, capacity, fill, doc_begin, doc_end, status, keep_zero_rows=False):
    """ops.store_append on CPU tensors, by the ABI's words rather than by the restatement above: a row is kept iff
    (bits & ~sign) != 0 somewhere in it."""
    assert x.dim() == 3 and fill.dtype == torch.int64 and status.dtype == torch.int32
    assert doc_begin.shape == doc_end.shape == (x.shape[0],) and doc_begin.is_contiguous() and doc_end.is_contiguous()
    assert rows_out is not None or codes_out is not None
    if int(status[0]) != 0:
        return
    mag = bits(x) & (0x7fffffff if x.dtype == torch.float32 else 0x7fff)
    keep = torch.ones(x.shape[:2], dtype=torch.bool) if keep_zero_rows else (mag != 0).any(-1)
    counts = keep.sum(1)
    f = int(fill[0])
    if f + int(counts.sum()) > capacity:
        status[0] = 1
        return
    kept = x[keep]
    n = kept.shape[0]
    if rows_out is not None:
        assert rows_out.dtype == x.dtype or torch.float32 in (rows_out.dtype, x.dtype)
        rows_out[f: f + n] = kept.to(rows_out.dtype)
    if codes_out is not None:
        c, s = R8.quantize_torch(kept)
        codes_out[f: f + n] = c
        scales_out[f: f + n] = s
    e = f + torch.cumsum(counts, 0)
    doc_end.copy_(e)
    doc_begin.copy_(e - counts)
    fill[0] = f + n


# ------------------------------------------------------------------------------------------ shared inputs
def _tiny(dtype):
    """The smallest subnormal of dtype."""
    return torch.tensor([1], dtype=_BITS[dtype]).view(dtype)[0]


_LIVE = {}


def _live_rows(n: int, E: int, dtype) -> torch.Tensor:
    """The first n of one seeded set of live rows per (E, dtype), generated once (the largest batch of the suite is reused)."""
    key = (E, dtype)
    if key not in _LIVE or _LIVE[key].shape[0] < n:
        x = torch.randn(max(n, 4096), E, generator=torch.Generator().manual_seed(1000 + E))
        x[:, 0] = x[:, 0].abs() + 0.5
        _LIVE[key] = x.to(dtype)
    return _LIVE[key][:n]


def pattern_batch(n_docs: int, D: int, E: int, dtype, seed: int, shift: int = 0) -> torch.Tensor:
    """x [n_docs, D, E] of dtype (CPU).  Document b follows pattern (b + shift) % 7:
      0 fully live;  1 all zero;  2 only the last row live;  3 a zero row between live rows (row D // 2; D = 1: the row);
      4 zero but for one row whose only non-zero element is one subnormal;  5 live but for a row of -0.0 only;
      6 a live prefix of seeded length, then zero padding (what a model's mask leaves).
    Live rows are seeded values of magnitude around 1 with a non-zero first element."""
    g = torch.Generator().manual_seed(seed)
    x = _live_rows(n_docs * D, E, dtype).view(n_docs, D, E).clone()
    pat = (torch.arange(n_docs) + shift) % 7
    lens = torch.randint(0, D + 1, (n_docs,), generator=g)
    j = torch.arange(D)[None, :]
    zero = (pat == 1)[:, None] | (pat == 4)[:, None] | ((pat == 2)[:, None] & (j < D - 1)) | ((pat == 3)[:, None] & (j == D // 2)) \
        | ((pat == 6)[:, None] & (j >= lens[:, None]))
    x[zero] = 0
    sub = torch.nonzero(pat == 4).flatten()
    if sub.numel():
        x[sub, (sub * 7) % D, (sub * 3) % E] = _tiny(dtype)
    neg = torch.nonzero(pat == 5).flatten()
    if neg.numel():
        x[neg, (neg * 5) % D] = torch.tensor(-0.0, dtype=dtype)
    return x
