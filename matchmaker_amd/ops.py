"""Host side of the scoring operators: torch tensors in, torch tensors out, arithmetic in
libmm_native.so (hand-written HIP, gfx950).  torch is used only for device memory and streams.

Every function launches on the *current* torch stream of the tensors' device, allocates only its
output (+ a small mask-packing workspace from torch's caching allocator), never synchronises and
keeps no state, so it is re-entrant from nn.DataParallel's per-GPU threads
(matchmaker/train.py:201).  CPU tensors are rejected: there is no CPU fallback.
"""
import ctypes
import threading
from typing import Optional

import torch

from . import _lib
from ._lib import NativeError

_DT = {torch.float32: _lib.MM_F32, torch.float16: _lib.MM_F16, torch.bfloat16: _lib.MM_BF16}


def _dev_check(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise NativeError("matchmaker_amd operators need HIP device tensors (got a CPU tensor); "
                              "there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise NativeError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def _emb(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype not in _DT:
        raise NativeError(f"{name}: unsupported dtype {t.dtype}")
    if t.dim() != 3:
        raise NativeError(f"{name}: expected [rows, tokens, dim], got {tuple(t.shape)}")
    return t.contiguous()


_NATIVE_DIMS = (128, 256, 384, 512, 768)      # the row widths the retrieval kernels are instantiated for


def _pair16(op: str, a: torch.Tensor, b: torch.Tensor, la: str, lb: str):
    """Two 2-D float16 / bfloat16 matrices of one dtype and one width; la / lb name their shapes in the message."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise NativeError(f"{op}: expected {la} and {lb}, got {tuple(a.shape)} {tuple(b.shape)}")
    if a.dtype != b.dtype or b.dtype not in (torch.float16, torch.bfloat16):
        raise NativeError(f"{op}: float16 / bfloat16 vectors of one dtype needed, got {a.dtype} / {b.dtype}")


def _native_width(op: str, E: int):
    if E not in _NATIVE_DIMS:
        raise NativeError(f"{op}: E={E} is not one of 128, 256, 384, 512, 768 (pad the vectors)", _lib.MM_EUNSUPPORTED)


def _list_begin_check(op: str, list_begin: torch.Tensor):
    if list_begin.dim() != 1 or list_begin.dtype != torch.int64 or list_begin.shape[0] < 2:
        raise NativeError(f"{op}: list_begin must be int64 [nlist + 1], got {list_begin.dtype} {tuple(list_begin.shape)}")


def _probes_check(op: str, probes: torch.Tensor, nq: int):
    if probes.dim() != 2 or probes.dtype != torch.int32 or probes.shape[0] != nq or probes.shape[1] < 1:
        raise NativeError(f"{op}: probes must be int32 [nq, nprobe], got {probes.dtype} {tuple(probes.shape)}")


def _k_range(op: str, k: int, nprobe: int):
    if not 1 <= k <= 4096 or nprobe > 4096:
        raise NativeError(f"{op}: k={k} / nprobe={nprobe} outside 1 .. 4096")


def _queries16(op: str, queries: torch.Tensor):
    if queries.dim() != 2 or queries.dtype not in _DT:
        raise NativeError(f"{op}: queries: expected [nq, E] float16 / bfloat16, got {tuple(queries.shape)} {queries.dtype}")


def _fp8_store(op: str, row: str, q: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> int:
    """The fp8 store of an operator and its query: codes [rows, E] uint8, scales [rows] float32, q fp16 or bf16.  `row` is
    the letter the operator's messages give the row count.  Returns the rows."""
    if q.dtype == torch.float32:
        raise NativeError(f"{op}: the query is fp16 or bf16 (convert it; an fp32 query has no exact 16-bit MFMA operand)",
                          _lib.MM_EUNSUPPORTED)
    if codes.dim() != 2 or codes.dtype != torch.uint8:
        raise NativeError(f"{op}: codes: expected [{row}, E] uint8, got {tuple(codes.shape)} {codes.dtype}")
    rows = codes.shape[0]
    if scales.dtype != torch.float32 or tuple(scales.shape) != (rows,):
        raise NativeError(f"{op}: scales: expected [{rows}] float32 (one per row of codes), got "
                          f"{tuple(scales.shape)} {scales.dtype}")
    return rows


def _topk_out(dev, nq: int, k: int):
    """The (scores [nq, k] float32, rows [nq, k] int64) pair the top-k operators return."""
    return torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)


def _pad_last(t: torch.Tensor, mult: int) -> torch.Tensor:
    E = t.shape[-1]
    return t if E % mult == 0 else torch.nn.functional.pad(t, (0, mult - E % mult))


def _pad_rows(q: torch.Tensor, d: torch.Tensor, mult: int):
    """Token rows must be 16-byte multiples for the native loads.  Zero columns change neither dot products nor
    norms, so other widths (KNRM on 50-d GloVe, colbert_compression_dim 100, ...) are padded up — a copy, taken
    only for such widths.  Returns (q, d, padded E)."""
    q, d = _pad_last(q, mult), _pad_last(d, mult)
    return q, d, q.shape[-1]


def _pad16(q: torch.Tensor, d: torch.Tensor):
    """_pad_rows to 16 bytes of the tensors' own element type."""
    return _pad_rows(q, d, 4 if q.dtype == torch.float32 else 8)


def _trim(g: Optional[torch.Tensor], E0: int) -> Optional[torch.Tensor]:
    """A gradient computed at the padded width, back at the E0 columns the caller passed (a copy, taken only when padded)."""
    return g if g is None or g.shape[-1] == E0 else g[..., :E0].contiguous()


def _mask(m: Optional[torch.Tensor], rows: int, L: int, name: str):
    """-> (tensor kept alive, pointer, kind)"""
    if m is None:
        return None, None, _lib.MASK_NONE
    if m.dim() == 1:
        if m.shape[0] != rows:
            raise NativeError(f"{name}: expected {rows} lengths, got {tuple(m.shape)}")
        m = m.to(torch.int32).contiguous()
        return m, m.data_ptr(), _lib.MASK_LEN_I32
    if tuple(m.shape) != (rows, L):
        raise NativeError(f"{name}: expected [{rows}, {L}], got {tuple(m.shape)}")
    if m.dtype == torch.int64:
        kind = _lib.MASK_I64
    elif m.dtype == torch.float32:
        kind = _lib.MASK_F32
    elif m.dtype in (torch.uint8, torch.bool):
        kind = _lib.MASK_U8
    else:
        m = (m != 0)
        kind = _lib.MASK_U8
    m = m.contiguous()
    return m, m.data_ptr(), kind


# The current stream's raw handle without building a torch.cuda.Stream object (~0.3 us instead of ~2.5: two of those per
# call were a fifth of the host time of a 512-pair call).  torch._C._cuda_getCurrentRawStream is what torch's own
# compiled-code launchers use; the public path stays as the fallback.
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev) -> int:
    if _RAW_STREAM is not None and dev.index is not None:
        return _RAW_STREAM(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


# Mask-packing workspaces of the scoring calls, one per (device, stream): calls on one stream are ordered, so the
# next call may reuse the buffer; eval.py-sized calls (512 pairs) are host-bound and a torch.empty per call is ~2 us
# of their ~15.  Not used under graph capture (a captured graph must not reference a buffer a later call may replace).
_WS = {}
_WS_LOCK = threading.Lock()      # nn.DataParallel drives forward() from one Python thread per GPU (train.py:201)


def _workspace(dev, nbytes: int, stream: Optional[int] = None):
    if nbytes == 0:
        return None
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev.index, _stream(dev) if stream is None else stream)
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        with _WS_LOCK:
            if len(_WS) > 64:
                _WS.clear()
            t = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
            _WS[key] = t
    return t


def clear_workspaces() -> None:
    """Drops the cached mask-packing workspaces (one per (device, stream) that ever called a scoring operator, sized for the
    largest call seen there, at most 64 of them): they are ordinary torch allocations, so torch.cuda.empty_cache() can
    return their memory afterwards.  Safe at any time — a call in flight holds its own reference."""
    with _WS_LOCK:
        _WS.clear()


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NOCTX = _NoCtx()


def _on(dev):
    """Device guard for the native call: torch's context manager costs ~2-3 us per call, which is visible on 512-pair
    calls; nothing to guard when `dev` already is the current device (the single-GPU-per-process case)."""
    return _NOCTX if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


_WSB = {}


def _ws_bytes(fn, *key):
    """Workspace size of a call shape (a pure function of the integers in `key`): one ctypes round trip per shape, not per call."""
    k = (fn.__name__,) + key
    v = _WSB.get(k)
    if v is None:
        if len(_WSB) > 4096:
            _WSB.clear()
        v = _WSB[k] = fn(*key)
    return v


def _vec(t: torch.Tensor) -> torch.Tensor:
    """A small parameter tensor as float32 contiguous memory.  Only its data pointer and element count are used, so a
    contiguous fp32 tensor of any shape is taken as it is — the models' own buffers / parameters (`mu` [1,1,1,K],
    `kernel_alpha_scaler` [1,1,K], `kernel_bin_weights.weight` [1,K]) cost no dispatch per call."""
    if t.dtype is torch.float32 and t.is_contiguous():
        return t
    return _flat32(t)


def _flat32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().reshape(-1).to(torch.float32).contiguous()


def _flags(sim_round: bool, sum_round: bool) -> int:
    return (_lib.SIM_ROUND if sim_round else 0) | (_lib.SUM_ROUND if sum_round else 0)


def _call(dev, fn, args, size_fn=None, key=(), cached=False, stream_only=False):
    """The native call every operator ends with: fn(*args, workspace pointer or None, workspace bytes, stream) under the
    device guard, on the current stream (its handle is read once), then the check of the return code under fn's name.
    size_fn(*key), key = integers, gives the workspace size (None: the entry point needs no workspace); cached: the workspace
    is the per-stream buffer of _workspace (host-bound calls), else a fresh allocation (large ones, which the cache would hold
    on to).  stream_only: the entry point's signature has no workspace arguments, fn(*args, stream)."""
    with _on(dev):
        st = _stream(dev)
        if stream_only:
            rc = fn(*args, st)
        else:
            wsb = _ws_bytes(size_fn, *key) if size_fn is not None else 0
            if cached:
                ws = _workspace(dev, wsb, st)
            else:
                ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
            rc = fn(*args, ws.data_ptr() if ws is not None else None, wsb, st)
    _lib.check(rc, fn.__name__)


# ---- checks the scoring operators share -------------------------------------------------------------------------------
def _same_dtype(q: torch.Tensor, d: torch.Tensor):
    if q.dtype != d.dtype:
        raise NativeError(f"q/d dtype mismatch: {q.dtype} vs {d.dtype}")


def _same_width(E: int, E2: int):
    if E != E2:
        raise NativeError(f"embedding dims differ: {E} vs {E2}")


def _per_query(nq: int, B: int, pairs_per_query: int):
    if pairs_per_query < 1 or nq != (B + pairs_per_query - 1) // pairs_per_query:
        raise NativeError(f"q has {nq} rows but {B} pairs / {pairs_per_query} per query")


def _qd_shapes(q: torch.Tensor, d: torch.Tensor, pairs_per_query: int):
    """q [n_queries, Q, E] against d [n_pairs, D, E], pairs_per_query pairs per query -> (nq, Q, E, B, D)."""
    nq, Q, E = q.shape
    B, D, E2 = d.shape
    _same_width(E, E2)
    _per_query(nq, B, pairs_per_query)
    return nq, Q, E, B, D


def _pair_per_row(op: str, q: torch.Tensor, d: torch.Tensor):
    """The layout of the backwards: q [B, Q, E], d [B, D, E] -> (B, Q, D, E)."""
    if q.shape[0] != d.shape[0] or q.shape[2] != d.shape[2]:
        raise NativeError(f"{op} needs the pair-per-row layout: q {tuple(q.shape)} vs d {tuple(d.shape)}")
    return q.shape[0], q.shape[1], d.shape[1], q.shape[2]


def _grad_flat(grad_out: torch.Tensor, n: int, pairs: str) -> torch.Tensor:
    go = _flat32(grad_out)
    if go.numel() != n:
        raise NativeError(f"grad_out has {go.numel()} elements for {pairs} pairs")
    return go


def _grad_dtype(op: str, grad_dtype: Optional[torch.dtype], q: torch.Tensor) -> torch.dtype:
    gdt = torch.float32 if grad_dtype is None else grad_dtype
    if gdt not in (torch.float32, q.dtype):
        raise NativeError(f"{op}: gradients are float32 or {q.dtype}, not {gdt}")
    return gdt


def reference_rounding(q: torch.Tensor) -> "tuple[bool, bool]":
    """(sim_round, sum_round) that reproduce what the reference's eager ops do with token vectors of q's dtype in the
    CURRENT autocast state: 16-bit vectors give a 16-bit similarity matrix (`bmm` / `mm`, the -1000 fill and `max`,
    colbert.py:68-71); `sum` (:75) is promoted to fp32 under autocast and is a 16-bit op outside it (the dynamic
    teacher's all-pairs call, dynamic_teacher.py:245-246).  fp32 vectors outside autocast: no rounding anywhere."""
    ac = torch.is_autocast_enabled("cuda")
    lowp = q.dtype in (torch.float16, torch.bfloat16)
    return (lowp or ac), (lowp and not ac)


def maxsim(q: torch.Tensor, d: torch.Tensor, q_mask: Optional[torch.Tensor] = None,
           d_mask: Optional[torch.Tensor] = None, pairs_per_query: int = 1, sim_round: bool = False,
           sum_round: bool = False) -> torch.Tensor:
    """ColBERT MaxSim (matchmaker/models/colbert.py:68-75; unmasked: :100-112).

    q [n_queries, Q, E], d [n_pairs, D, E]; pair p scores against query p // pairs_per_query.
    Masks: None | 1-D lengths | [rows, L] bool/uint8/int64/float (nonzero = real token).
    sim_round / sum_round: the reference's dtype flow for fp16 / bf16 vectors (MM_SIM_ROUND / MM_SUM_ROUND in
    include/mm_native.h): per-token maxima rounded to the vectors' dtype before the fp32 sum (what autocast does,
    colbert.py:60-75), and the sum as well (16-bit tensors outside autocast).  Default: fp32 through max and sum.
    Returns float32 [n_pairs] (with sum_round the values are exactly representable in the vectors' dtype)."""
    dev = _dev_check(q, d, q_mask, d_mask)
    q, d = _emb(q, "q"), _emb(d, "d")
    _same_dtype(q, d)
    nq, Q, E, B, D = _qd_shapes(q, d, pairs_per_query)
    qm, qp, qk = _mask(q_mask, nq, Q, "q_mask")
    dm, dp, dk = _mask(d_mask, B, D, "d_mask")
    L = _lib.lib()
    out = torch.empty(B, dtype=torch.float32, device=dev)
    if B == 0:
        return out
    q, d, E = _pad16(q, d)
    _call(dev, L.mm_maxsim_fwd, (q.data_ptr(), d.data_ptr(), qp, qk, dp, dk, out.data_ptr(), B, pairs_per_query, Q, D, E,
                                 _DT[q.dtype], _flags(sim_round, sum_round)),
          L.mm_maxsim_workspace_bytes, (B, pairs_per_query, Q, D, qk, dk), cached=True)
    return out


class _MaxsimBatch(ctypes.Structure):      # mm_maxsim_batch_t (include/mm_native.h)
    _fields_ = [("q", ctypes.c_void_p), ("d", ctypes.c_void_p), ("q_mask", ctypes.c_void_p), ("d_mask", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("n_pairs", ctypes.c_int64)]


MAXSIM_MAX_BATCHES = 16


def maxsim_batched(batches, sim_round: bool = False, sum_round: bool = False):
    """Several pair-per-row batches of ONE shape scored by one launch (mm_maxsim_fwd_batched): `batches` = a sequence of
    (q [B, Q, E], d [B, D, E], q_mask, d_mask) with 16-bit vectors and either int64 tokenizer masks ([B, Q] / [B, D]) or None for
    both, everywhere.  Returns the list of float32 score tensors [B] (views of one allocation), bit-equal to maxsim() on
    each batch.  Raises NativeError(MM_EUNSUPPORTED ...) for shapes the pair-per-row kernel does not take (callers fall back
    to one maxsim() per batch); more than MAXSIM_MAX_BATCHES batches go out in several launches."""
    batches = list(batches)
    if not batches:
        return []
    q0, d0, qm0, dm0 = batches[0]
    dev = _dev_check(*[t for b in batches for t in b])
    Q, E, D = q0.shape[1], q0.shape[2], d0.shape[1]
    has_masks = qm0 is not None
    total = sum(b[1].shape[0] for b in batches)
    out = torch.empty(total, dtype=torch.float32, device=dev)
    L = _lib.lib()
    keep, views, recs, off = [], [], [], 0
    for q, d, qm, dm in batches:
        q, d = _emb(q, "q"), _emb(d, "d")
        if q.dtype != q0.dtype or d.dtype != q0.dtype or q.dtype == torch.float32:
            raise NativeError("maxsim_batched: 16-bit vectors of one dtype in every batch")
        if q.shape[1:] != (Q, E) or d.shape[1:] != (D, E) or q.shape[0] != d.shape[0]:
            raise NativeError(f"maxsim_batched: every batch must be pair-per-row [B, {Q}, {E}] / [B, {D}, {E}], got {tuple(q.shape)} / {tuple(d.shape)}")
        if (qm is not None) != has_masks or (dm is not None) != has_masks:
            raise NativeError("maxsim_batched: masks for every batch or for none")
        B = d.shape[0]
        if has_masks:
            if qm.dtype != torch.int64 or dm.dtype != torch.int64 or tuple(qm.shape) != (B, Q) or tuple(dm.shape) != (B, D):
                raise NativeError("maxsim_batched: masks are the tokenizer's int64 [B, Q] / [B, D] tensors")
            qm, dm = qm.contiguous(), dm.contiguous()
        keep.append((q, d, qm, dm))
        o = out[off:off + B]
        views.append(o)
        recs.append(_MaxsimBatch(q.data_ptr(), d.data_ptr(), qm.data_ptr() if has_masks else None,
                                 dm.data_ptr() if has_masks else None, o.data_ptr(), B))
        off += B
    kind = _lib.MASK_I64 if has_masks else _lib.MASK_NONE
    with _on(dev):
        st = _stream(dev)
        for i in range(0, len(recs), MAXSIM_MAX_BATCHES):
            part = recs[i:i + MAXSIM_MAX_BATCHES]
            arr = (_MaxsimBatch * len(part))(*part)
            rc = L.mm_maxsim_fwd_batched(ctypes.cast(arr, ctypes.c_void_p), len(part), kind, kind, Q, D, E, _DT[q0.dtype],
                                         _flags(sim_round, sum_round), st)
            _lib.check(rc, "mm_maxsim_fwd_batched")
    return views


def hbm_stream_probe(t: torch.Tensor, nt: bool = True) -> None:
    """Calibration launch (mm_hbm_stream_probe): streams tensor `t` through the MaxSim kernel's LDS-DMA ring with the
    arithmetic removed.  Returns nothing: it exists to be timed (bench.py extra.hbm_calibration)."""
    dev = _dev_check(t)
    t = t.contiguous()
    nbytes = (t.numel() * t.element_size()) // 8192 * 8192
    _call(dev, _lib.lib().mm_hbm_stream_probe, (t.data_ptr(), nbytes, 1 if nt else 0), stream_only=True)


def _check_ranges(doc_begin: torch.Tensor, doc_end: torch.Tensor, n_rows: int):
    """A stale doc_infos range (another store's, or past the token matrix) would make the LDS-DMA stream read out of
    bounds silently.  A device reduction + one blocking D2H read: callers that validated their ranges when they built
    them (token_store.TokenStore does, on the host copy of doc_infos) pass check_ranges=False and keep the launch
    stream free of synchronisation."""
    if torch.cuda.is_current_stream_capturing():
        raise NativeError("maxsim_ragged: range validation needs a D2H read; validate outside graph capture and pass "
                          "check_ranges=False")
    lo, hi = int(doc_begin.min()), int(torch.maximum(doc_begin, doc_end).max())
    bad = int((doc_begin > doc_end).sum())
    if lo < 0 or hi > n_rows or bad:
        raise NativeError(f"maxsim_ragged: document ranges [{lo}, {hi}) leave the {n_rows}-row token matrix"
                          + (f" ({bad} ranges have begin > end)" if bad else ""))


def _maxsim_ragged(dev, fn, size_fn, q, store, n_rows, doc_begin, doc_end, q_mask, pairs_per_query, check_ranges, flags):
    """What maxsim_ragged and maxsim_ragged_fp8 share once their store is validated: `store` = the store's tensors in the
    order the entry point `fn` takes them, n_rows = its token rows."""
    nq, Q, E = q.shape
    B = doc_begin.numel()
    if doc_end.numel() != B:
        raise NativeError("doc_begin / doc_end must have one entry per pair")
    _per_query(nq, B, pairs_per_query)
    doc_begin = doc_begin.to(torch.int64).contiguous()
    doc_end = doc_end.to(torch.int64).contiguous()
    qm, qp, qk = _mask(q_mask, nq, Q, "q_mask")
    out = torch.empty(B, dtype=torch.float32, device=dev)
    if B == 0:
        return out
    if check_ranges:
        _check_ranges(doc_begin, doc_end, n_rows)
    _call(dev, fn, (q.data_ptr(), *[t.data_ptr() for t in store], doc_begin.data_ptr(), doc_end.data_ptr(), qp, qk,
                    out.data_ptr(), B, pairs_per_query, Q, E, _DT[q.dtype], flags), size_fn, (B, pairs_per_query, Q, qk))
    return out


def maxsim_ragged(q: torch.Tensor, tokens: torch.Tensor, doc_begin: torch.Tensor, doc_end: torch.Tensor,
                  q_mask: Optional[torch.Tensor] = None, pairs_per_query: int = 1,
                  check_ranges: bool = True, sim_round: bool = False, sum_round: bool = False) -> torch.Tensor:
    """Unpadded MaxSim over a resident token store (the ColBERT retrieval aggregate,
    matchmaker/dense_retrieval.py:398-412 + colbert.py:100-112, in ONE launch).

    q [n_queries, Q, E]; tokens [T, E] (the store: token_reps_N.npy rows); document p of the batch is
    tokens[doc_begin[p]:doc_end[p]] (doc_infos ranges); pair p scores against query
    p // pairs_per_query.  Returns float32 [n_pairs]."""
    dev = _dev_check(q, tokens, doc_begin, doc_end, q_mask)
    q = _emb(q, "q")
    if tokens.dim() != 2 or tokens.dtype not in _DT:
        raise NativeError(f"tokens: expected [T, E] float tensor, got {tuple(tokens.shape)} {tokens.dtype}")
    if q.dtype != tokens.dtype:
        raise NativeError(f"q/tokens dtype mismatch: {q.dtype} vs {tokens.dtype} (convert the query to the store's dtype)")
    tokens = tokens.contiguous()
    _same_width(q.shape[2], tokens.shape[1])
    L = _lib.lib()
    return _maxsim_ragged(dev, L.mm_maxsim_ragged_fwd, L.mm_maxsim_ragged_workspace_bytes, q, (tokens,), tokens.shape[0],
                          doc_begin, doc_end, q_mask, pairs_per_query, check_ranges, _flags(sim_round, sum_round))


def fp8_quantize_rows(x: torch.Tensor) -> "tuple[torch.Tensor, torch.Tensor]":
    """Token rows -> the fp8 store format (mm_fp8_quantize_rows, include/mm_native.h): x [T, E] fp16 / bf16 / fp32 with
    E % 16 == 0 -> (codes [T, E] uint8 = OCP e4m3fn bytes, scales [T] float32 = one power of two per row); the row's value is
    deq(code) * scale.  Deterministic (no atomics).  Non-finite input is the caller's error."""
    dev = _dev_check(x)
    if x.dim() != 2 or x.dtype not in _DT:
        raise NativeError(f"fp8_quantize_rows: expected [T, E] float tensor, got {tuple(x.shape)} {x.dtype}")
    T, E = x.shape
    if E % 16:
        raise NativeError(f"fp8_quantize_rows: E={E} is not a multiple of 16", _lib.MM_EUNSUPPORTED)
    x = x.contiguous()
    codes = torch.empty((T, E), dtype=torch.uint8, device=dev)
    scales = torch.empty(T, dtype=torch.float32, device=dev)
    if T == 0:
        return codes, scales
    _call(dev, _lib.lib().mm_fp8_quantize_rows, (x.data_ptr(), T, E, _DT[x.dtype], codes.data_ptr(), scales.data_ptr()),
          stream_only=True)
    return codes, scales


def fp8_dequantize_rows(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The values an fp8 store holds, deq(codes) * scales[:, None], in `dtype` — plain torch, on the tensors' device (CPU
    included).  Exact in float32; exact in bfloat16 / float16 too unless the product leaves that type's range (every e4m3
    value has 4 significant bits and the scale is a power of two)."""
    if codes.dtype != torch.uint8 or codes.dim() != 2 or scales.shape != (codes.shape[0],):
        raise NativeError(f"fp8_dequantize_rows: expected codes [T, E] uint8 and scales [T], got {tuple(codes.shape)} "
                          f"{codes.dtype} / {tuple(scales.shape)}")
    return (codes.view(torch.float8_e4m3fn).to(torch.float32) * scales.to(torch.float32)[:, None]).to(dtype)


def maxsim_ragged_fp8(q: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, doc_begin: torch.Tensor,
                      doc_end: torch.Tensor, q_mask: Optional[torch.Tensor] = None, pairs_per_query: int = 1,
                      check_ranges: bool = True, sim_round: bool = False, sum_round: bool = False) -> torch.Tensor:
    """maxsim_ragged over an fp8 token store (mm_maxsim_ragged_fp8_fwd): codes [T, E] uint8 + scales [T] float32 as
    fp8_quantize_rows writes them, q [n_queries, Q, E] fp16 or bf16 (NOT quantised: the codes are converted to q's type in
    registers, exactly, and the row scale multiplies the finished fp32 dot product).  Document p is rows
    [doc_begin[p], doc_end[p]); pair p scores against query p // pairs_per_query.  sim_round / sum_round round to q's
    dtype as in maxsim_ragged.  Returns float32 [n_pairs]."""
    dev = _dev_check(q, codes, scales, doc_begin, doc_end, q_mask)
    q = _emb(q, "q")
    T = _fp8_store("maxsim_ragged_fp8", "T", q, codes, scales)
    E = q.shape[2]
    _same_width(E, codes.shape[1])
    if E % 16:
        raise NativeError(f"maxsim_ragged_fp8: E={E} is not a multiple of 16", _lib.MM_EUNSUPPORTED)
    L = _lib.lib()
    return _maxsim_ragged(dev, L.mm_maxsim_ragged_fp8_fwd, L.mm_maxsim_ragged_fp8_workspace_bytes, q,
                          (codes.contiguous(), scales.contiguous()), T, doc_begin, doc_end, q_mask, pairs_per_query,
                          check_ranges, _flags(sim_round, sum_round))


def maxsim_bwd(q: torch.Tensor, d: torch.Tensor, q_mask: Optional[torch.Tensor], d_mask: Optional[torch.Tensor],
               grad_out: torch.Tensor, grad_dtype: Optional[torch.dtype] = None):
    """Backward of the paired MaxSim (pair-per-row layout).  Returns (grad_q [B,Q,E], grad_d [B,D,E]) as float32, or —
    grad_dtype = q.dtype — in the token vectors' own 16-bit type (what autograd hands back to an fp16 / bf16 encoder:
    one launch, summed in fp32, rounded once); see mm_maxsim_bwd in include/mm_native.h."""
    dev = _dev_check(q, d, q_mask, d_mask, grad_out)
    q, d = _emb(q, "q"), _emb(d, "d")
    _same_dtype(q, d)
    B, Q, D, E0 = _pair_per_row("maxsim_bwd", q, d)
    go = _grad_flat(grad_out, B, f"{B}")
    qm, qp, qk = _mask(q_mask, B, Q, "q_mask")
    dm, dp, dk = _mask(d_mask, B, D, "d_mask")
    L = _lib.lib()
    q, d, E = _pad16(q, d)
    gdt = _grad_dtype("maxsim_bwd", grad_dtype, q)
    gq = torch.empty((B, Q, E), dtype=gdt, device=dev)
    gd = torch.empty((B, D, E), dtype=gdt, device=dev)
    if B:
        _call(dev, L.mm_maxsim_bwd, (q.data_ptr(), d.data_ptr(), qp, qk, dp, dk, go.data_ptr(), gq.data_ptr(), gd.data_ptr(),
                                     _DT[gdt], B, Q, D, E, _DT[q.dtype]),
              L.mm_maxsim_bwd_workspace_bytes, (B, Q, D, qk, dk), cached=True)
    return _trim(gq, E0), _trim(gd, E0)


def maxsim_inbatch(q: torch.Tensor, q_mask: Optional[torch.Tensor], d: torch.Tensor,
                   d_mask: Optional[torch.Tensor], bug_compatible: bool = False, sim_round: bool = False,
                   sum_round: bool = False) -> torch.Tensor:
    """All-pairs MaxSim [Bq, Bd] (matchmaker/models/colbert.py:154-162).  bug_compatible=True masks
    score[i, j] with document i's mask as the reference does (and needs Bq == Bd).  sim_round / sum_round as in
    maxsim() (the dynamic teacher calls this on fp16 vectors outside autocast: both, dynamic_teacher.py:245-246)."""
    dev = _dev_check(q, d, q_mask, d_mask)
    q, d = _emb(q, "q"), _emb(d, "d")
    _same_dtype(q, d)
    Bq, Q, E = q.shape
    Bd, D, E2 = d.shape
    _same_width(E, E2)
    qm, qp, qk = _mask(q_mask, Bq, Q, "q_mask")
    dm, dp, dk = _mask(d_mask, Bd, D, "d_mask")
    L = _lib.lib()
    out = torch.empty((Bq, Bd), dtype=torch.float32, device=dev)
    if Bq == 0 or Bd == 0:
        return out
    q, d, E = _pad16(q, d)
    _call(dev, L.mm_maxsim_inbatch_fwd, (q.data_ptr(), d.data_ptr(), qp, qk, dp, dk, out.data_ptr(), Bq, Bd, Q, D, E,
                                         _DT[q.dtype], 1 if bug_compatible else 0, _flags(sim_round, sum_round)),
          L.mm_maxsim_inbatch_workspace_bytes, (Bq, Bd, Q, D, qk, dk))
    return out


def maxsim_inbatch_bwd(q: torch.Tensor, q_mask: Optional[torch.Tensor], d: torch.Tensor, d_mask: Optional[torch.Tensor],
                       grad_out: torch.Tensor, bug_compatible: bool = False, grad_dtype: Optional[torch.dtype] = None,
                       need_q: bool = True, need_d: bool = True):
    """Backward of the all-pairs MaxSim (colbert.py:154-162; in-batch negatives, train.py:434-467).  grad_out [Bq, Bd];
    returns (grad_q [Bq,Q,E], grad_d [Bd,D,E]) as float32, or — grad_dtype = q.dtype — in the token vectors' own 16-bit type
    (summed in fp32, rounded once).  First arg-max on ties, no floating-point atomics: two calls give the same bits; see
    mm_maxsim_inbatch_bwd in include/mm_native.h.  need_q / need_d = False: that gradient's pass is not run and None stands
    in its place (a frozen encoder)."""
    dev = _dev_check(q, d, q_mask, d_mask, grad_out)
    q, d = _emb(q, "q"), _emb(d, "d")
    _same_dtype(q, d)
    Bq, Q, E0 = q.shape
    Bd, D, E2 = d.shape
    _same_width(E0, E2)
    if bug_compatible and Bq != Bd:
        raise NativeError(f"maxsim_inbatch_bwd: bug_compatible masking (colbert.py:158) requires Bq == Bd (got {Bq}, {Bd})",
                          _lib.MM_EINVAL)
    go = _grad_flat(grad_out, Bq * Bd, f"{Bq} x {Bd}")
    qm, qp, qk = _mask(q_mask, Bq, Q, "q_mask")
    dm, dp, dk = _mask(d_mask, Bd, D, "d_mask")
    L = _lib.lib()
    q, d, E = _pad16(q, d)
    gdt = _grad_dtype("maxsim_inbatch_bwd", grad_dtype, q)
    gq = torch.empty((Bq, Q, E), dtype=gdt, device=dev) if need_q else None
    gd = torch.empty((Bd, D, E), dtype=gdt, device=dev) if need_d else None
    if Bq == 0 or Bd == 0:
        return (gq.zero_()[..., :E0] if need_q else None), (gd.zero_()[..., :E0] if need_d else None)
    if not (need_q or need_d):
        return None, None
    _call(dev, L.mm_maxsim_inbatch_bwd, (q.data_ptr(), d.data_ptr(), qp, qk, dp, dk, go.data_ptr(),
                                         gq.data_ptr() if need_q else None, gd.data_ptr() if need_d else None, _DT[gdt],
                                         Bq, Bd, Q, D, E, _DT[q.dtype], 1 if bug_compatible else 0),
          L.mm_maxsim_inbatch_bwd_workspace_bytes, (Bq, Bd, Q, D, E, qk, dk), cached=True)
    return _trim(gq, E0), _trim(gd, E0)


def kernel_pool(q: torch.Tensor, d: torch.Tensor, q_mask: Optional[torch.Tensor], d_mask: Optional[torch.Tensor],
                mu: torch.Tensor, sigma: torch.Tensor, alpha: torch.Tensor, w: torch.Tensor,
                pairs_per_query: int = 1, return_per_kernel: bool = False,
                d_gate: Optional[torch.Tensor] = None, clamp_min: float = 1e-10,
                pair_query: Optional[torch.Tensor] = None, return_pooled: bool = False):
    """TK kernel pooling (matchmaker/models/published/ecai20_tk.py:105-124).

    q [n_queries, Q, E], d [n_pairs, D, E] float32 contextualised embeddings; mu/sigma/alpha/w [K].
    d_gate [n_pairs, D] >= 0 (optional): TK-Sparse's stop-word vector (cikm20_tk_sparse.py:133-135);
    clamp_min: floor inside the log (1e-4: IDCM sampler, sigir21_idcm.py:185);
    pair_query [n_pairs] int (optional): row of q each pair scores against (ragged groups; replaces
    pairs_per_query; equal neighbours reuse the query tile).
    Returns float32 [n_pairs] (and per_kernel [n_pairs, K] when asked; and, with return_pooled, the pooled kernel sums
    [n_pairs, Q, K] of :120 as the LAST element — what kernel_pool_bwd(pooled=...) takes to skip its pooling pre-pass; rows of
    padded query tokens are unspecified)."""
    dev = _dev_check(q, d, q_mask, d_mask, mu, sigma, alpha, w, d_gate, pair_query)
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError("kernel_pool: float32 embeddings only (the reference cosine rejects bf16, "
                          "and tk.yaml sets use_fp16: False)")
    nq, Q, E = q.shape
    B, D, E2 = d.shape
    _same_width(E, E2)
    if pair_query is not None:
        pq = pair_query.reshape(-1).to(torch.int32).contiguous()
        if pq.numel() != B:
            raise NativeError(f"pair_query has {pq.numel()} entries for {B} pairs")
        if B and not torch.cuda.is_current_stream_capturing():
            lo, hi = int(pq.min()), int(pq.max())
            if lo < 0 or hi >= nq:
                raise NativeError(f"pair_query values [{lo}, {hi}] outside the {nq} query rows")
        pairs_per_query = 1
    else:
        _per_query(nq, B, pairs_per_query)
        pq = None
    K = mu.numel()
    mu, sigma, alpha, w = _vec(mu), _vec(sigma), _vec(alpha), _vec(w)
    if not (sigma.numel() == alpha.numel() == w.numel() == K):
        raise NativeError("kernel_pool: mu/sigma/alpha/w must all have K elements")
    qm, qp, qk = _mask(q_mask, nq, Q, "q_mask")
    dm, dp, dk = _mask(d_mask, B, D, "d_mask")
    gate = _gate(d_gate, B, D)
    L = _lib.lib()
    out = torch.empty(B, dtype=torch.float32, device=dev)
    pk = torch.empty((B, K), dtype=torch.float32, device=dev) if return_per_kernel else None
    pooled = torch.empty((B, Q, K), dtype=torch.float32, device=dev) if return_pooled else None
    if B:
        q, d, E = _pad_rows(q, d, 4)
        _call(dev, L.mm_kernel_pool_ex_fwd2, (q.data_ptr(), d.data_ptr(), qp, qk, dp, dk,
                                              gate.data_ptr() if gate is not None else None,
                                              pq.data_ptr() if pq is not None else None, nq, mu.data_ptr(),
                                              sigma.data_ptr(), alpha.data_ptr(), w.data_ptr(), float(clamp_min),
                                              out.data_ptr(), pk.data_ptr() if pk is not None else None,
                                              pooled.data_ptr() if pooled is not None else None, B,
                                              pairs_per_query, Q, D, E, K, _lib.MM_F32),
              L.mm_kernel_pool_workspace_bytes, (max(B, nq), pairs_per_query, Q, D, qk, dk), cached=True)
    res = (out, pk) if return_per_kernel else (out,)
    if return_pooled:
        res = res + (pooled,)
    return res if len(res) > 1 else out


def kernel_pool_multi(q_list, d_list, q_mask: Optional[torch.Tensor], d_mask: Optional[torch.Tensor], mu: torch.Tensor,
                      sigma: torch.Tensor, alpha: torch.Tensor, w: torch.Tensor, clamp_min: float = 1e-10) -> torch.Tensor:
    """Sum over all (i, t) of kernel_pool(q_list[i], d_list[t], bin weights w[i * len(d_list) + t]) in ONE launch
    (+ a deterministic sum): Conv-KNRM's n_grams^2 match matrices and its dense layer (conv_knrm.py:130-137).
    q_list[i] [B, Q, E], d_list[t] [B, D, E] float32 (pair-per-row), w [len(q_list) * len(d_list), K].  Returns [B]."""
    q_list = [_emb(t, "q") for t in q_list]
    d_list = [_emb(t, "d") for t in d_list]
    dev = _dev_check(*q_list, *d_list, q_mask, d_mask, mu, sigma, alpha, w)
    B, Q, E = q_list[0].shape
    D = d_list[0].shape[1]
    for t in q_list:
        if tuple(t.shape) != (B, Q, E) or t.dtype != torch.float32:
            raise NativeError(f"kernel_pool_multi: query tensors must all be float32 [{B},{Q},{E}]")
    for t in d_list:
        if tuple(t.shape) != (B, D, E) or t.dtype != torch.float32:
            raise NativeError(f"kernel_pool_multi: document tensors must all be float32 [{B},{D},{E}]")
    nq_, nd_ = len(q_list), len(d_list)
    K = mu.numel()
    mu, sigma, alpha, w = _vec(mu), _vec(sigma), _vec(alpha), _vec(w)
    if w.numel() != nq_ * nd_ * K or sigma.numel() != K or alpha.numel() != K:
        raise NativeError("kernel_pool_multi: w must hold K weights per (query tensor, document tensor) combination")
    q_list = [_pad_last(t, 4) for t in q_list]
    d_list = [_pad_last(t, 4) for t in d_list]
    E = q_list[0].shape[-1]
    qm, qp, qk = _mask(q_mask, B, Q, "q_mask")
    dm, dp, dk = _mask(d_mask, B, D, "d_mask")
    L = _lib.lib()
    out = torch.empty(B, dtype=torch.float32, device=dev)
    if B == 0:
        return out
    qa = (ctypes.c_void_p * nq_)(*[t.data_ptr() for t in q_list])
    da = (ctypes.c_void_p * nd_)(*[t.data_ptr() for t in d_list])
    _call(dev, L.mm_kernel_pool_multi_fwd, (ctypes.cast(qa, ctypes.c_void_p), nq_, ctypes.cast(da, ctypes.c_void_p), nd_, qp, qk,
                                            dp, dk, mu.data_ptr(), sigma.data_ptr(), alpha.data_ptr(), w.data_ptr(),
                                            float(clamp_min), out.data_ptr(), B, 1, Q, D, E, K, _lib.MM_F32),
          L.mm_kernel_pool_multi_workspace_bytes, (B, 1, nq_, nd_, Q, D, qk, dk))
    return out


def _gate(d_gate, B, D):
    if d_gate is None:
        return None
    g = d_gate.detach().reshape(B, -1).to(torch.float32).contiguous()
    if g.shape[1] != D:
        raise NativeError(f"d_gate has shape {tuple(d_gate.shape)} for {B} documents of {D} tokens")
    return g


def kernel_pool_bwd(q: torch.Tensor, d: torch.Tensor, q_mask: Optional[torch.Tensor], d_mask: Optional[torch.Tensor],
                    mu: torch.Tensor, sigma: torch.Tensor, alpha: torch.Tensor, w: torch.Tensor, grad_out: torch.Tensor,
                    d_gate: Optional[torch.Tensor] = None, clamp_min: float = 1e-10, pooled: Optional[torch.Tensor] = None):
    """Backward of kernel_pool in the pair-per-row layout (mm_kernel_pool_ex_bwd2).  Returns float32
    (grad_q [B,Q,E], grad_d [B,D,E], grad_alpha [K], grad_w [K]) and, with d_gate, grad_gate [B,D] as a
    fifth element.  pooled [B,Q,K]: the forward's pooled kernel sums (kernel_pool(..., return_pooled=True) on the same inputs);
    without them the backward pools them itself first (the document crosses HBM twice)."""
    dev = _dev_check(q, d, q_mask, d_mask, mu, sigma, alpha, w, grad_out, d_gate, pooled)
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError("kernel_pool_bwd: float32 embeddings only")
    B, Q, D, E0 = _pair_per_row("kernel_pool_bwd", q, d)
    K = mu.numel()
    mu, sigma, alpha, w = _vec(mu), _vec(sigma), _vec(alpha), _vec(w)
    go = _grad_flat(grad_out, B, f"{B}")
    qm, qp, qk = _mask(q_mask, B, Q, "q_mask")
    dm, dp, dk = _mask(d_mask, B, D, "d_mask")
    L = _lib.lib()
    q, d, E = _pad_rows(q, d, 4)
    gq = torch.empty((B, Q, E), dtype=torch.float32, device=dev)
    gd = torch.empty((B, D, E), dtype=torch.float32, device=dev)
    gaw = torch.zeros((2, B, K), dtype=torch.float32, device=dev)    # per-pair rows of grad_alpha, grad_w: one memset, one sum
    ga, gw = gaw[0], gaw[1]
    gate = _gate(d_gate, B, D)
    gg = torch.zeros((B, D), dtype=torch.float32, device=dev) if gate is not None else None
    if pooled is not None:
        if pooled.dtype != torch.float32 or tuple(pooled.shape) != (B, Q, K):
            raise NativeError(f"pooled has shape {tuple(pooled.shape)} / {pooled.dtype}, expected float32 {(B, Q, K)}")
        pooled = pooled.detach().contiguous()
    if B:
        _call(dev, L.mm_kernel_pool_ex_bwd2, (q.data_ptr(), d.data_ptr(), qp, qk, dp, dk,
                                              gate.data_ptr() if gate is not None else None, mu.data_ptr(),
                                              sigma.data_ptr(), alpha.data_ptr(), w.data_ptr(), float(clamp_min),
                                              pooled.data_ptr() if pooled is not None else None,
                                              go.data_ptr(), gq.data_ptr(), gd.data_ptr(),
                                              gg.data_ptr() if gg is not None else None, ga.data_ptr(), gw.data_ptr(),
                                              B, Q, D, E, K),
              L.mm_kernel_pool_bwd_workspace_bytes2, (B, Q, D, E, qk, dk))
    gq, gd = _trim(gq, E0), _trim(gd, E0)
    gaw = gaw.sum(1)
    if gate is not None:
        return gq, gd, gaw[0], gaw[1], gg
    return gq, gd, gaw[0], gaw[1]


def tkl_score(q_ctx: torch.Tensor, chunks: torch.Tensor, chunk_mask: torch.Tensor, chunk_slot: torch.Tensor,
              q_mask: torch.Tensor, params: torch.Tensor, B: int, C: int, K: int, saturation: str = "embedding",
              return_windows: bool = False, check_order: bool = True, return_peaks: bool = False):
    """TKL windowed kernel pooling + region top-k (sigir20_tkl.py:180-286).  See mm_native.h.

    return_peaks: also return the region search's three arg-max window indices per document, int64 [B, 3] in round order =
    the reference's `top_non_overlapping_idx` (:266-271).  Returns score | (score, win) | (score, win, peaks).

    chunk_slot must be strictly ASCENDING (what boolean-mask packing / torch.nonzero produce, sigir20_tkl.py:159-162): the
    kernels rely on a document's chunks being adjacent and on its last kept chunk coming last.  check_order=True verifies
    that on the device without a host synchronisation (torch._assert_async: a violation raises at the next
    synchronisation point instead of silently zeroing live windows); callers that built chunk_slot with
    tkl.chunk_documents() — the drop-in does — pass False and skip the three small launches."""
    dev = _dev_check(q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params)
    q_ctx, chunks = _emb(q_ctx, "q_ctx"), _emb(chunks, "chunks")
    if q_ctx.dtype != torch.float32 or chunks.dtype != torch.float32:
        raise NativeError("tkl_score: float32 only (tkl.yaml use_fp16: False)")
    Bq, Q, E = q_ctx.shape
    P = chunks.shape[0]
    if Bq != B or chunks.shape[1] != 50 or chunks.shape[2] != E:
        raise NativeError(f"tkl_score: bad shapes q_ctx {tuple(q_ctx.shape)} chunks {tuple(chunks.shape)}")
    sat = {"embedding": _lib.TKL_SAT_EMBEDDING, "log": _lib.TKL_SAT_LOG}.get(saturation)
    if sat is None:
        raise NativeError(f"tkl_score: saturation {saturation!r} is dead code in the reference "
                          "(reads the undefined `query_idfs`, sigir20_tkl.py:214,236)")
    chunk_mask = chunk_mask.to(torch.float32).contiguous()
    chunk_slot = chunk_slot.to(torch.int32).contiguous()
    if check_order and P > 1 and not torch.cuda.is_current_stream_capturing():
        torch._assert_async((chunk_slot[1:] > chunk_slot[:-1]).all(),
                            "tkl_score: chunk_slot must be strictly ascending (include/mm_native.h, mm_tkl_fwd)")
    q_mask = q_mask.to(torch.float32).contiguous()
    params = params.to(torch.float32).contiguous()
    W = (max(C * 40, 30) - 30) // 2 + 1
    L = _lib.lib()
    out = torch.empty(B, dtype=torch.float32, device=dev)
    win = torch.empty((B, W), dtype=torch.float32, device=dev)
    peaks = torch.empty((B, 3), dtype=torch.int32, device=dev) if return_peaks else None
    if B:
        _call(dev, L.mm_tkl_fwd_peaks, (q_ctx.data_ptr(), chunks.data_ptr(), chunk_mask.data_ptr(), chunk_slot.data_ptr(),
                                        q_mask.data_ptr(), params.data_ptr(), win.data_ptr(), out.data_ptr(),
                                        peaks.data_ptr() if peaks is not None else None, B, P, C, Q, E, K, sat),
              L.mm_tkl_workspace_bytes, (B, P, C, Q, K))
    if return_peaks:
        return out, win, peaks.long()
    return (out, win) if return_windows else out


def tkl_bwd(q_ctx: torch.Tensor, chunks: torch.Tensor, chunk_mask: torch.Tensor, chunk_slot: torch.Tensor,
            q_mask: torch.Tensor, params: torch.Tensor, win: torch.Tensor, grad_out: torch.Tensor, B: int, C: int, K: int,
            saturation: str = "embedding"):
    """Backward of tkl_score (mm_tkl_bwd): returns float32 (grad_q_ctx [B,Q,E], grad_chunks [P,50,E],
    grad_params [MM_TKL_NPARAMS] summed over the documents, in the layout of `params`)."""
    dev = _dev_check(q_ctx, chunks, chunk_mask, chunk_slot, q_mask, params, win, grad_out)
    q_ctx, chunks = _emb(q_ctx.detach(), "q_ctx"), _emb(chunks.detach(), "chunks")
    if q_ctx.dtype != torch.float32 or chunks.dtype != torch.float32:
        raise NativeError("tkl_bwd: float32 only")
    Bq, Q, E = q_ctx.shape
    P = chunks.shape[0]
    sat = {"embedding": _lib.TKL_SAT_EMBEDDING, "log": _lib.TKL_SAT_LOG}.get(saturation)
    if sat is None or Bq != B or (P and (chunks.shape[1] != 50 or chunks.shape[2] != E)):
        raise NativeError(f"tkl_bwd: bad arguments (saturation {saturation!r}, q_ctx {tuple(q_ctx.shape)}, chunks {tuple(chunks.shape)})")
    chunk_mask = chunk_mask.to(torch.float32).contiguous()
    chunk_slot = chunk_slot.to(torch.int32).contiguous()
    q_mask = q_mask.to(torch.float32).contiguous()
    params = params.detach().to(torch.float32).contiguous()
    win = win.detach().to(torch.float32).contiguous()
    go = _flat32(grad_out)
    NP = params.numel()
    gq = torch.empty((B, Q, E), dtype=torch.float32, device=dev)
    gc = torch.empty((P, 50, E), dtype=torch.float32, device=dev)
    gp = torch.empty((B, NP), dtype=torch.float32, device=dev)
    if B == 0:
        return gq, gc.zero_(), torch.zeros(NP, dtype=torch.float32, device=dev)
    L = _lib.lib()
    _call(dev, L.mm_tkl_bwd, (q_ctx.data_ptr(), chunks.data_ptr() if P else None, chunk_mask.data_ptr() if P else None,
                              chunk_slot.data_ptr() if P else None, q_mask.data_ptr(), params.data_ptr(), win.data_ptr(),
                              go.data_ptr(), gq.data_ptr(), gc.data_ptr() if P else None, gp.data_ptr(), B, P, C, Q, E, K, sat),
          L.mm_tkl_bwd_workspace_bytes2, (B, C, Q, E))
    return gq, gc, gp.sum(0)


def _topk_reruns(name: str, dev, fn, size_fn, queries: torch.Tensor, store, k: int, max_rounds: int):
    """The status-driven loop of the flat top-k operators (dot_topk, dot_topk_fp8): one native call over every query, then
    re-runs of the queries whose sampled threshold let too few / too many candidates through, with the threshold scale
    bisected per query.  fn = the entry point, store = the tensors it takes between the queries and the row count (the
    first one has a row per store row); every run gets a fresh workspace of size_fn(N, n, k) bytes."""
    nq, E = queries.shape
    N = store[0].shape[0]
    out_s, out_i = _topk_out(dev, nq, k)
    if nq == 0:
        return out_s, out_i
    if N == 0:
        return out_s.fill_(float("-inf")), out_i.fill_(-1)

    def run(q, scale, s=None, i=None):
        n = q.shape[0]
        if s is None:
            s, i = _topk_out(dev, n, k)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        _call(dev, fn, (q.data_ptr(), *[t.data_ptr() for t in store], N, n, E, _DT[q.dtype], k, scale, s.data_ptr(),
                        i.data_ptr(), st.data_ptr()), size_fn, (N, n, k))
        return s, i, st

    _, _, st = run(queries, 1.0, out_s, out_i)        # straight into the caller's tensors (no 84 MB staging copy)
    if int(st.max()) == 0:                            # one 4-byte D2H: the exactness check of the status vector
        return out_s, out_i
    bad = torch.nonzero(st != 0).flatten().tolist()
    # rare path: bisect the threshold scale per query (status 1 = too few survivors -> larger m,
    # status 2 = candidate list overflowed -> smaller m)
    codes = st[bad].tolist()
    lo = {q: (1.0 if c == 1 else None) for q, c in zip(bad, codes)}   # largest scale known to underflow
    hi = {q: (1.0 if c == 2 else None) for q, c in zip(bad, codes)}   # smallest scale known to overflow
    for _ in range(max_rounds):
        groups = {}
        for q in bad:
            if lo[q] is not None and hi[q] is not None:
                sc = (lo[q] * hi[q]) ** 0.5
            else:
                sc = lo[q] * 4.0 if lo[q] is not None else hi[q] * 0.25
            groups.setdefault(round(sc, 6), []).append(q)
        still = []
        for sc, qs in groups.items():
            sel = torch.tensor(qs, dtype=torch.int64, device=dev)
            s2, i2, st2 = run(queries[sel].contiguous(), float(sc))
            st2 = st2.tolist()
            for n, q in enumerate(qs):
                if st2[n] == 0:
                    out_s[q] = s2[n]
                    out_i[q] = i2[n]
                else:
                    if st2[n] == 1:
                        lo[q] = sc
                    else:
                        hi[q] = sc
                    still.append(q)
        bad = still
        if not bad:
            return out_s, out_i
    raise NativeError(f"{name}: {len(bad)} queries without an exact top-{k} after {max_rounds} threshold re-runs "
                      "(more than 4k documents tie at the k-th score?)")


def dot_topk(queries: torch.Tensor, corpus: torch.Tensor, k: int, max_rounds: int = 6):
    """Exact brute-force inner-product top-k over one shard (faiss IndexFlatIP.search semantics;
    matchmaker/retrieval/faiss_indices.py:22-36, :49-74; score = bert_dot.py:62).

    queries [nq, E], corpus [N, E] float16 / bfloat16 on the same device, E in {128,...,768} (pad
    otherwise).  Returns (scores [nq, k] float32 descending, idx [nq, k] int64 rows of `corpus`,
    -1 / -inf padded when N < k).  The native call thresholds every query from a sample of the
    shard; queries whose threshold let too few / too many candidates through (status != 0, rare)
    are re-run with a moved threshold until every row is exact."""
    dev = _dev_check(queries, corpus)
    _pair16("dot_topk", queries, corpus, "[nq, E]", "[N, E]")
    queries, corpus = queries.contiguous(), corpus.contiguous()
    L = _lib.lib()
    return _topk_reruns("dot_topk", dev, L.mm_dot_topk_fwd, L.mm_dot_topk_workspace_bytes, queries, (corpus,), k, max_rounds)


def dot_topk_fp8(queries: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, k: int, max_rounds: int = 6):
    """dot_topk over an fp8 token store (mm_dot_topk_fp8_fwd): codes [N, E] uint8 + scales [N] float32 as fp8_quantize_rows
    writes them, queries [nq, E] fp16 or bf16 (NOT quantised: the codes are converted to the query's type in registers,
    exactly, and the row scale multiplies the finished fp32 dot product).  score[q, t] = scales[t] * <queries[q],
    deq(codes[t])>.  E in {128, 256, 384, 512, 768}.  Returns (scores [nq, k] float32 descending, idx [nq, k] int64 rows
    of the store, -1 / -inf padded when N < k); equal scores go to the lower row; the same status-driven re-runs as
    dot_topk make every row exact."""
    dev = _dev_check(queries, codes, scales)
    _queries16("dot_topk_fp8", queries)
    _fp8_store("dot_topk_fp8", "N", queries, codes, scales)
    _same_width(queries.shape[1], codes.shape[1])
    L = _lib.lib()
    return _topk_reruns("dot_topk_fp8", dev, L.mm_dot_topk_fp8_fwd, L.mm_dot_topk_fp8_workspace_bytes, queries.contiguous(),
                        (codes.contiguous(), scales.contiguous()), k, max_rounds)


def ivf_scan(queries: torch.Tensor, vectors: torch.Tensor, list_begin: torch.Tensor, probes: torch.Tensor, k: int):
    """Exact inner-product top-k over the inverted lists each query probes (the list scan of an IVF index:
    matchmaker/retrieval/faiss_indices.py:106-145; native mm_ivf_scan_fwd).

    queries [nq, E], vectors [n, E] float16 / bfloat16 of one dtype, E in {128,...,768} (pad otherwise); the vectors are
    stored list by list, list l = rows list_begin[l] .. list_begin[l + 1] (list_begin [nlist + 1] int64).  probes
    [nq, nprobe] int32 list numbers, -1 = no list.  A list named twice in one row is a caller error that is not detected:
    the result of that row is then undefined (copies of a vector may be returned, or lists dropped; memory stays in
    bounds).  Returns (scores [nq, k] float32 descending,
    rows [nq, k] int64 rows of `vectors`; -inf / -1 padded when the probed lists hold fewer than k vectors; equal scores:
    lower row first).  One enqueue on the current stream, no read-back: graph-capturable."""
    dev = _dev_check(queries, vectors, list_begin, probes)
    _pair16("ivf_scan", queries, vectors, "[nq, E]", "[n, E]")
    _list_begin_check("ivf_scan", list_begin)
    _probes_check("ivf_scan", probes, queries.shape[0])
    _k_range("ivf_scan", k, probes.shape[1])
    queries, vectors = queries.contiguous(), vectors.contiguous()
    list_begin, probes = list_begin.contiguous(), probes.contiguous()
    nq, E = queries.shape
    n, nlist, nprobe = vectors.shape[0], list_begin.shape[0] - 1, probes.shape[1]
    out_s, out_r = _topk_out(dev, nq, k)
    if nq == 0:
        return out_s, out_r
    L = _lib.lib()
    _call(dev, L.mm_ivf_scan_fwd, (queries.data_ptr(), vectors.data_ptr() if n else None, list_begin.data_ptr(),
                                   probes.data_ptr(), n, nlist, nq, nprobe, E, _DT[queries.dtype], k, out_s.data_ptr(),
                                   out_r.data_ptr()),
          L.mm_ivf_scan_workspace_bytes, (n, nlist, nq, nprobe, k), cached=True)
    return out_s, out_r


def ivf_scan_fp8(queries: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, list_begin: torch.Tensor,
                 probes: torch.Tensor, k: int):
    """ivf_scan over lists held as an fp8 token store (mm_ivf_scan_fp8_fwd; the same reference lines as ivf_scan):
    codes [n, E] uint8 + scales [n] float32 as fp8_quantize_rows writes them, stored list by list (list l = rows
    list_begin[l] .. list_begin[l + 1]); queries [nq, E] fp16 or bf16 (NOT quantised: the codes are converted to the
    query's type in registers, exactly, and the row scale multiplies the finished fp32 dot product).  score[q, t] =
    scales[t] * <queries[q], deq(codes[t])> for every row t of the lists in probes[q] ([nq, nprobe] int32, -1 = no list; a
    list named twice in one row: undefined result, memory stays in bounds).  E in {128, 256, 384, 512, 768}.  Returns
    (scores [nq, k] float32 descending, rows [nq, k] int64 rows of `codes`; -inf / -1 padded when the probed lists hold
    fewer than k rows; equal scores: lower row first).  One enqueue on the current stream, no read-back: graph-capturable."""
    dev = _dev_check(queries, codes, scales, list_begin, probes)
    _queries16("ivf_scan_fp8", queries)
    n = _fp8_store("ivf_scan_fp8", "n", queries, codes, scales)
    nq, E = queries.shape
    _same_width(E, codes.shape[1])
    _native_width("ivf_scan_fp8", E)
    _list_begin_check("ivf_scan_fp8", list_begin)
    _probes_check("ivf_scan_fp8", probes, nq)
    _k_range("ivf_scan_fp8", k, probes.shape[1])
    queries, codes, scales = queries.contiguous(), codes.contiguous(), scales.contiguous()
    list_begin, probes = list_begin.contiguous(), probes.contiguous()
    nlist, nprobe = list_begin.shape[0] - 1, probes.shape[1]
    out_s, out_r = _topk_out(dev, nq, k)
    if nq == 0:
        return out_s, out_r
    L = _lib.lib()
    _call(dev, L.mm_ivf_scan_fp8_fwd, (queries.data_ptr(), codes.data_ptr() if n else None, scales.data_ptr() if n else None,
                                       list_begin.data_ptr(), probes.data_ptr(), n, nlist, nq, nprobe, E, _DT[queries.dtype], k,
                                       out_s.data_ptr(), out_r.data_ptr()),
          L.mm_ivf_scan_fp8_workspace_bytes, (n, nlist, nq, nprobe, k), cached=True)
    return out_s, out_r


def _ah_codebook_check(what: str, codebook: torch.Tensor, E: int, dtype):
    if codebook.dim() != 3 or tuple(codebook.shape) != (E // 2, 16, 2) or codebook.dtype != dtype:
        raise NativeError(f"{what}: codebook must be {dtype} [{E // 2}, 16, 2], got {codebook.dtype} {tuple(codebook.shape)}")
    return codebook.contiguous()


def ah_encode(x: torch.Tensor, lists: torch.Tensor, centroids: torch.Tensor, codebook: torch.Tensor, eta: float, passes: int = 2):
    """Anisotropic 4-bit codes of 2-dimensional blocks (the encoder of a quantized index, faiss_index_type: scann:
    matchmaker/retrieval/scann_index.py:24-47, `score_ah(2, anisotropic_quantization_threshold)`; native mm_ah_encode).

    x [n, E], centroids [nlist, E], codebook [E / 2, 16, 2] float16 / bfloat16 of one dtype, E in {128,...,768} (pad
    otherwise); lists [n] int32 = the leaf of every row.  Per row the residual to its leaf centre is coded block by block:
    the nearest codeword first, then `passes` ascending sweeps of coordinate descent on
    sum |e_s|^2 + (eta - 1) (sum <e_s, x / |x|>)^2 (include/mm_native.h states every fp32 step); lowest code on equal cost.
    Returns codes [n, E / 4] uint8, the even block in the low nibble.  A pure function of the inputs (no atomics); one
    enqueue on the current stream, no workspace, no read-back: graph-capturable."""
    dev = _dev_check(x, lists, centroids, codebook)
    _pair16("ah_encode", x, centroids, "[n, E]", "[nlist, E]")
    n, E = x.shape
    _native_width("ah_encode", E)
    if lists.dim() != 1 or lists.dtype != torch.int32 or lists.shape[0] != n:
        raise NativeError(f"ah_encode: lists must be int32 [n], got {lists.dtype} {tuple(lists.shape)}")
    if centroids.shape[0] < 1:
        raise NativeError("ah_encode: no centroids")
    codebook = _ah_codebook_check("ah_encode", codebook, E, x.dtype)
    eta, passes = float(eta), int(passes)
    if not (0.0 <= eta < 3.0e38) or not 0 <= passes <= 64:
        raise NativeError(f"ah_encode: eta={eta} must be finite and >= 0, passes={passes} in 0 .. 64", _lib.MM_EUNSUPPORTED)
    x, lists, centroids = x.contiguous(), lists.contiguous(), centroids.contiguous()
    codes = torch.empty((n, E // 4), dtype=torch.uint8, device=dev)
    if n == 0:
        return codes
    _call(dev, _lib.lib().mm_ah_encode, (x.data_ptr(), lists.data_ptr(), centroids.data_ptr(), codebook.data_ptr(), n,
                                         centroids.shape[0], E, _DT[x.dtype], eta, passes, codes.data_ptr()), stream_only=True)
    return codes


def ah_scan(queries: torch.Tensor, codes: torch.Tensor, codebook: torch.Tensor, list_begin: torch.Tensor, probes: torch.Tensor,
            probe_scores: torch.Tensor, k: int):
    """Exact top-k of the quantized scores over the lists each query probes (the 4-bit scoring stage of a quantized index,
    faiss_index_type: scann: matchmaker/retrieval/scann_index.py:24-47; native mm_ah_scan_fwd).

    queries [nq, E] float16 / bfloat16, E in {128,...,768}; codes [n, E / 4] uint8 stored list by list, list l = rows
    list_begin[l] .. list_begin[l + 1] (list_begin [nlist + 1] int64); codebook [E / 2, 16, 2] of the queries' dtype; probes
    [nq, nprobe] int32 list numbers, -1 = no list (a list named twice in one row: undefined result, memory stays in
    bounds); probe_scores [nq, nprobe] float32.  score(q, i) = probe_scores[q, j] + <q, decode(codes[i])> for row i of list
    probes[q, j], fp32-accumulated.  Returns (scores [nq, k] float32 descending, rows [nq, k] int64; -inf / -1 padded;
    equal scores: lower row first).  One enqueue on the current stream, no read-back: graph-capturable."""
    dev = _dev_check(queries, codes, codebook, list_begin, probes, probe_scores)
    if queries.dim() != 2 or codes.dim() != 2 or queries.shape[1] != codes.shape[1] * 4 or codes.dtype != torch.uint8:
        raise NativeError(f"ah_scan: expected [nq, E] queries and uint8 [n, E / 4] codes, got {tuple(queries.shape)} "
                          f"{codes.dtype} {tuple(codes.shape)}")
    if queries.dtype not in (torch.float16, torch.bfloat16):
        raise NativeError(f"ah_scan: float16 / bfloat16 queries needed, got {queries.dtype}")
    nq, E = queries.shape
    _native_width("ah_scan", E)
    codebook = _ah_codebook_check("ah_scan", codebook, E, queries.dtype)
    _list_begin_check("ah_scan", list_begin)
    _probes_check("ah_scan", probes, nq)
    if probe_scores.dtype != torch.float32 or tuple(probe_scores.shape) != tuple(probes.shape):
        raise NativeError(f"ah_scan: probe_scores must be float32 {tuple(probes.shape)}, got {probe_scores.dtype} "
                          f"{tuple(probe_scores.shape)}")
    _k_range("ah_scan", k, probes.shape[1])
    queries, codes, list_begin = queries.contiguous(), codes.contiguous(), list_begin.contiguous()
    probes, probe_scores = probes.contiguous(), probe_scores.contiguous()
    n, nlist, nprobe = codes.shape[0], list_begin.shape[0] - 1, probes.shape[1]
    out_s, out_r = _topk_out(dev, nq, k)
    if nq == 0:
        return out_s, out_r
    L = _lib.lib()
    _call(dev, L.mm_ah_scan_fwd, (queries.data_ptr(), codes.data_ptr() if n else None, codebook.data_ptr(), list_begin.data_ptr(),
                                  probes.data_ptr(), probe_scores.data_ptr(), n, nlist, nq, nprobe, E, _DT[queries.dtype], k,
                                  out_s.data_ptr(), out_r.data_ptr()),
          L.mm_ah_scan_workspace_bytes, (n, nlist, nq, nprobe, k), cached=True)
    return out_s, out_r


def gather_dot(queries: torch.Tensor, vectors: torch.Tensor, rows: torch.Tensor):
    """Exact inner products of every query with the rows named for it (the re-score of a quantized index's candidates:
    matchmaker/retrieval/scann_index.py:35 `reorder`; native mm_gather_dot).

    queries [nq, E], vectors [n, E] float16 / bfloat16 of one dtype, E in {128,...,768} (pad otherwise); rows [nq, R] int64,
    -1 = none.  Returns out [nq, R] float32 = <queries[q], vectors[rows[q, j]]> accumulated in fp32, -inf for a row of -1.
    One enqueue on the current stream, no workspace, no read-back: graph-capturable."""
    dev = _dev_check(queries, vectors, rows)
    _pair16("gather_dot", queries, vectors, "[nq, E]", "[n, E]")
    nq, E = queries.shape
    _native_width("gather_dot", E)
    if rows.dim() != 2 or rows.dtype != torch.int64 or rows.shape[0] != nq:
        raise NativeError(f"gather_dot: rows must be int64 [nq, R], got {rows.dtype} {tuple(rows.shape)}")
    queries, vectors, rows = queries.contiguous(), vectors.contiguous(), rows.contiguous()
    R = rows.shape[1]
    out = torch.empty((nq, R), dtype=torch.float32, device=dev)
    if nq == 0 or R == 0:
        return out
    _call(dev, _lib.lib().mm_gather_dot, (queries.data_ptr(), vectors.data_ptr() if vectors.shape[0] else None, rows.data_ptr(),
                                          vectors.shape[0], nq, R, E, _DT[queries.dtype], out.data_ptr()), stream_only=True)
    return out


def graph_search(queries: torch.Tensor, vectors: torch.Tensor, neighbors: torch.Tensor, entry_rows: torch.Tensor, ef: int, k: int,
                 width: int = 4, max_iters: Optional[int] = None, return_stats: bool = False):
    """Beam search over a fixed-degree neighbour graph (the search of a graph index, faiss_index_type: hnsw; native
    mm_graph_search_fwd).

    queries [nq, E], vectors [n, E] float16 / bfloat16 of one dtype (widths that are no multiple of 128 are zero-padded
    here: a copy of both); neighbors [n, M] int32 rows of `vectors`, -1 = none, M even in 2 .. 128; entry_rows
    [nq, n_entry] int32, -1 and duplicates ignored, 1 <= n_entry <= ef.  Per query the candidate list starts as the scored
    entry rows and keeps the best ef (1 .. 2048); at most max_iters times (None: ceil(ef / width) + 8) the `width`
    (1 .. 8) best entries not yet expanded are expanded: their unvisited neighbours are scored and merged.  Returns
    (scores [nq, k] float32 descending, rows [nq, k] int64; lower row first on equal scores; -inf / -1 where fewer than k
    rows were reached), and with return_stats also stats [nq, 2] int32 = (iterations run, rows scored).  One enqueue on
    the current stream, no read-back: graph-capturable."""
    dev = _dev_check(queries, vectors, neighbors, entry_rows)
    _pair16("graph_search", queries, vectors, "[nq, E]", "[n, E]")
    if neighbors.dim() != 2 or neighbors.dtype != torch.int32 or neighbors.shape[0] != vectors.shape[0]:
        raise NativeError(f"graph_search: neighbors must be int32 [n, M], got {neighbors.dtype} {tuple(neighbors.shape)}")
    if entry_rows.dim() != 2 or entry_rows.dtype != torch.int32 or entry_rows.shape[0] != queries.shape[0]:
        raise NativeError(f"graph_search: entry_rows must be int32 [nq, n_entry], got {entry_rows.dtype} {tuple(entry_rows.shape)}")
    nq, E = queries.shape
    n, M, n_entry = vectors.shape[0], neighbors.shape[1], entry_rows.shape[1]
    if max_iters is None:
        max_iters = -(-int(ef) // max(1, int(width))) + 8
    if E % 128:
        queries, vectors, E = _pad_rows(queries, vectors, 128)
    queries, vectors = queries.contiguous(), vectors.contiguous()
    neighbors, entry_rows = neighbors.contiguous(), entry_rows.contiguous()
    out_s, out_r = _topk_out(dev, nq, max(int(k), 0))
    stats = torch.empty((nq, 2), dtype=torch.int32, device=dev) if return_stats else None
    if nq == 0:
        return (out_s, out_r, stats) if return_stats else (out_s, out_r)
    L = _lib.lib()
    _call(dev, L.mm_graph_search_fwd, (queries.data_ptr(), vectors.data_ptr(), neighbors.data_ptr(), entry_rows.data_ptr(), n, nq,
                                       E, _DT[queries.dtype], M, n_entry, int(ef), int(width), int(max_iters), int(k),
                                       out_s.data_ptr(), out_r.data_ptr(), stats.data_ptr() if return_stats else None),
          L.mm_graph_search_workspace_bytes, (n, nq, M, int(ef), int(width), n_entry, int(max_iters)), cached=True)
    return (out_s, out_r, stats) if return_stats else (out_s, out_r)


def kmeans_assign(x: torch.Tensor, centroids: torch.Tensor):
    """Maximum-inner-product assignment against a centroid table (the coarse quantiser of an IVF index with nprobe = 1:
    matchmaker/retrieval/faiss_indices.py:401-428, the loop of matchmaker/distillation/query_clusterer.py:218-221; native
    mm_kmeans_assign).

    x [n, E], centroids [nlist, E] float16 / bfloat16 of one dtype, E in {128,...,768} (pad otherwise), 1 <= nlist <= 65536.
    Returns (list [n] int32, score [n] float32 = the fp32-accumulated inner product with that centroid); equal scores: the
    lowest centroid number.  One enqueue on the current stream, no workspace, no read-back: graph-capturable."""
    dev = _dev_check(x, centroids)
    _pair16("kmeans_assign", x, centroids, "[n, E]", "[nlist, E]")
    n, E = x.shape
    nlist = centroids.shape[0]
    _native_width("kmeans_assign", E)
    if not 1 <= nlist <= 65536 or n >= 1 << 31:
        raise NativeError(f"kmeans_assign: nlist={nlist} outside 1 .. 65536, or n={n} >= 2^31", _lib.MM_EUNSUPPORTED)
    x, centroids = x.contiguous(), centroids.contiguous()
    out_l = torch.empty(n, dtype=torch.int32, device=dev)
    out_s = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out_l, out_s
    _call(dev, _lib.lib().mm_kmeans_assign, (x.data_ptr(), centroids.data_ptr(), n, nlist, E, _DT[x.dtype], out_l.data_ptr(),
                                             out_s.data_ptr()), stream_only=True)
    return out_l, out_s


def kmeans_segment_sum(x: torch.Tensor, order: torch.Tensor, list_begin: torch.Tensor):
    """Per-list fp32 sums of rows (the centroid update of k-means; native mm_kmeans_segment_sum).

    x [n, E] float16 / bfloat16, E in {128,...,768}; order [n] int64 = the rows of x list by list; list_begin [nlist + 1]
    int64, non-decreasing (lists may be empty).  Returns sums [nlist, E] float32, sums[l] = the sum of x[order[j]] for
    list_begin[l] <= j < list_begin[l + 1]; zeros for an empty list; rows of `order` outside [0, n) are skipped.  No
    atomics: the result is a pure function of the inputs, bit-equal run to run.  Enqueued on the current stream, no
    read-back: graph-capturable."""
    dev = _dev_check(x, order, list_begin)
    if x.dim() != 2 or x.dtype not in (torch.float16, torch.bfloat16):
        raise NativeError(f"kmeans_segment_sum: expected float16 / bfloat16 [n, E], got {x.dtype} {tuple(x.shape)}")
    if order.dim() != 1 or order.dtype != torch.int64 or order.shape[0] != x.shape[0]:
        raise NativeError(f"kmeans_segment_sum: order must be int64 [n], got {order.dtype} {tuple(order.shape)}")
    _list_begin_check("kmeans_segment_sum", list_begin)
    n, E = x.shape
    nlist = list_begin.shape[0] - 1
    _native_width("kmeans_segment_sum", E)
    if nlist > 65536 or n >= 1 << 31:
        raise NativeError(f"kmeans_segment_sum: nlist={nlist} outside 1 .. 65536, or n={n} >= 2^31", _lib.MM_EUNSUPPORTED)
    x, order, list_begin = x.contiguous(), order.contiguous(), list_begin.contiguous()
    sums = torch.empty((nlist, E), dtype=torch.float32, device=dev)
    L = _lib.lib()
    _call(dev, L.mm_kmeans_segment_sum, (x.data_ptr() if n else None, order.data_ptr() if n else None, list_begin.data_ptr(), n,
                                         nlist, E, _DT[x.dtype], sums.data_ptr()),
          L.mm_kmeans_segment_sum_workspace_bytes, (n, nlist, E), cached=True)
    return sums


def topk_merge(scores: torch.Tensor, ids: torch.Tensor, k: int):
    """Rows of (score, id) candidates [nq, n_in] -> the k best per row (score descending, input order on
    ties); ids < 0 are padding.  The sharded index's final merge (mm_topk_merge)."""
    dev = _dev_check(scores, ids)
    scores = scores.to(torch.float32).contiguous()
    ids = ids.to(torch.int64).contiguous()
    nq, n_in = scores.shape
    out_s, out_i = _topk_out(dev, nq, k)
    if nq:
        _call(dev, _lib.lib().mm_topk_merge, (scores.data_ptr(), ids.data_ptr(), nq, n_in, k, out_s.data_ptr(), out_i.data_ptr()),
              stream_only=True)
    return out_s, out_i


COLBERT_MAX_HITS = 16384      # hits per query of mm_colbert_candidates (64 KB of int32 keys in LDS) = mm_topk_merge's n_in limit


def colbert_candidates(hit_rows: torch.Tensor, begin_sorted: torch.Tensor, end_sorted: torch.Tensor,
                       doc_of_sorted: torch.Tensor, T: int, c_cap: Optional[int] = None):
    """Token hits -> candidate documents (the step between the token search and the aggregate of ColBERT retrieval,
    matchmaker/dense_retrieval.py:391-412 + colbert.py:100-112; native mm_colbert_candidates).

    hit_rows [nq, H] int64 rows of a T-row token matrix (-1 = no hit; rows outside [0, T) or owned by no document are
    dropped); begin_sorted / end_sorted [n_docs] int64 = the documents' row ranges sorted by (begin, end), non-empty ranges
    disjoint; doc_of_sorted [n_docs] int32 = the document index of every sorted range.  c_cap (default and minimum:
    min(H, n_docs)) = slots per query.  Returns (cand_doc [nq, c_cap] int32 ascending then -1, cand_begin, cand_end
    [nq, c_cap] int64 then (0, 0), count [nq] int32).  One enqueue on the current stream, no read-back: graph-capturable."""
    dev = _dev_check(hit_rows, begin_sorted, end_sorted, doc_of_sorted)
    if hit_rows.dim() != 2 or hit_rows.dtype != torch.int64:
        raise NativeError(f"colbert_candidates: hit_rows must be int64 [nq, H], got {hit_rows.dtype} {tuple(hit_rows.shape)}")
    n_docs = begin_sorted.numel()
    if (begin_sorted.dim() != 1 or end_sorted.shape != begin_sorted.shape or doc_of_sorted.shape != begin_sorted.shape
            or begin_sorted.dtype != torch.int64 or end_sorted.dtype != torch.int64 or doc_of_sorted.dtype != torch.int32):
        raise NativeError("colbert_candidates: begin_sorted / end_sorted must be int64 [n_docs] and doc_of_sorted int32 [n_docs], "
                          f"got {begin_sorted.dtype} {tuple(begin_sorted.shape)}, {end_sorted.dtype} {tuple(end_sorted.shape)}, "
                          f"{doc_of_sorted.dtype} {tuple(doc_of_sorted.shape)}")
    nq, H = hit_rows.shape
    if not 1 <= H <= COLBERT_MAX_HITS:
        raise NativeError(f"colbert_candidates: {H} hits per query outside 1 .. {COLBERT_MAX_HITS}", _lib.MM_EUNSUPPORTED)
    if not 1 <= n_docs < 2 ** 31:
        raise NativeError(f"colbert_candidates: {n_docs} documents outside 1 .. 2^31-1", _lib.MM_EUNSUPPORTED)
    need = min(H, n_docs)
    c_cap = need if c_cap is None else int(c_cap)
    if c_cap < need:
        raise NativeError(f"colbert_candidates: c_cap={c_cap} is below min(H, n_docs)={need}", _lib.MM_EUNSUPPORTED)
    hit_rows = hit_rows.contiguous()
    begin_sorted = begin_sorted.contiguous()
    end_sorted = end_sorted.contiguous()
    doc_of_sorted = doc_of_sorted.contiguous()
    cand_doc = torch.empty((nq, c_cap), dtype=torch.int32, device=dev)
    cand_begin = torch.empty((nq, c_cap), dtype=torch.int64, device=dev)
    cand_end = torch.empty((nq, c_cap), dtype=torch.int64, device=dev)
    count = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq == 0:
        return cand_doc, cand_begin, cand_end, count
    L = _lib.lib()
    _call(dev, L.mm_colbert_candidates, (hit_rows.data_ptr(), begin_sorted.data_ptr(), end_sorted.data_ptr(),
                                         doc_of_sorted.data_ptr(), n_docs, int(T), nq, H, c_cap, cand_doc.data_ptr(),
                                         cand_begin.data_ptr(), cand_end.data_ptr(), count.data_ptr()),
          L.mm_colbert_candidates_workspace_bytes, (nq, H), cached=True)
    return cand_doc, cand_begin, cand_end, count


DISTINCT_MAX_HITS = _lib.DISTINCT_MAX_HITS      # hits per query of mm_distinct_hits_fwd (128 KB of 16-byte keys in LDS)


def distinct_hits(scores: torch.Tensor, ids: torch.Tensor, top_n: int):
    """Passage hits -> distinct documents (matchmaker/dense_retrieval.py:414-429; native mm_distinct_hits_fwd): see
    matchmaker_amd/maxp.py, where the torch <-> ABI wrapper lives as the losses' lives in losses.py (a module of its own that
    tests/poison.py can be pointed at; the poisoned-memory case of this operator is in tests/test_maxp_gpu.py)."""
    from . import maxp
    return maxp.distinct_hits(scores, ids, top_n)


def inbatch_dot_loss(Q, Dp, Dn, sp, Tp, Tn, family, kind, need_grad=True, return_scores=False):
    """In-batch negatives from the vectors: loss, statistics and every gradient (matchmaker/train.py:434-472; native
    mm_inbatch_dot_loss_fwd): see matchmaker_amd/inbatch.py, where the torch <-> ABI wrapper lives as the losses' lives in
    losses.py (the poisoned-memory case of this operator is in tests/test_inbatch_gpu.py)."""
    from . import inbatch
    return inbatch.inbatch_dot_loss(Q, Dp, Dn, sp, Tp, Tn, family, kind, need_grad=need_grad, return_scores=return_scores)


def self_attention(qkv: torch.Tensor, mask: Optional[torch.Tensor], num_heads: int) -> torch.Tensor:
    """The attention core of the TK-family contextualiser on the in-projection as it lies in memory (ecai20_tk.py:138,
    sigir20_tkl.py:296-308, sigir21_idcm.py:174-175; native mm_self_attention_fwd): see matchmaker_amd/contextualize.py, where the
    torch <-> ABI wrapper lives (the poisoned-memory case of this operator is in tests/test_contextualize_gpu.py)."""
    from . import contextualize
    return contextualize.self_attention(qkv, mask, num_heads)


def store_append(x: torch.Tensor, rows_out: Optional[torch.Tensor], codes_out: Optional[torch.Tensor],
                 scales_out: Optional[torch.Tensor], capacity: int, fill: torch.Tensor, doc_begin: torch.Tensor,
                 doc_end: torch.Tensor, status: torch.Tensor, keep_zero_rows: bool = False) -> None:
    """A batch of encoder output -> its non-zero token rows appended to a resident store (the host half of the encode loop,
    matchmaker/dense_retrieval.py:232-265; native mm_store_append, include/mm_native.h).

    x [n_docs, D, E] fp16 / bf16 / fp32.  A row is kept iff it has an element of non-zero magnitude (keep_zero_rows: every
    row); the kept rows go back to back, document by document, to store rows fill[0] .. of
      rows_out [>= capacity, E] (x's dtype: the bits; fp32 -> fp16 / bf16 rounded to nearest even; fp16 / bf16 -> fp32), and / or
      codes_out [>= capacity, E] uint8 + scales_out [>= capacity] float32 = fp8_quantize_rows of the kept rows;
    doc_begin / doc_end [n_docs] int64 receive the documents' row ranges, fill [1] int64 advances, status [1] int32 is set to
    1 (and stays: later calls do nothing) when a batch does not fit below `capacity` — such a batch writes nothing at all.
    The five buffers are written in place, so they must be contiguous tensors (or contiguous slices) of the device.  Three
    launches on the current stream, no read-back: appends chain through `fill` and can be captured into a graph."""
    dev = _dev_check(x, rows_out, codes_out, scales_out, fill, doc_begin, doc_end, status)
    if x.dim() != 3 or x.dtype not in _DT:
        raise NativeError(f"store_append: x: expected [n_docs, D, E] fp16 / bf16 / fp32, got {tuple(x.shape)} {x.dtype}")
    n_docs, D, E = x.shape
    capacity = int(capacity)
    if rows_out is None and codes_out is None and scales_out is None:
        raise NativeError("store_append: neither rows_out nor codes_out / scales_out given", _lib.MM_EINVAL)
    if (codes_out is None) != (scales_out is None):
        raise NativeError("store_append: codes_out and scales_out go together", _lib.MM_EINVAL)
    if D < 1 or E < 1 or capacity < 0:
        raise NativeError(f"store_append: bad shape {tuple(x.shape)} / capacity {capacity}", _lib.MM_EINVAL)
    if rows_out is not None:
        if rows_out.dtype not in _DT or rows_out.dim() != 2 or rows_out.shape[1] != E or rows_out.shape[0] < capacity:
            raise NativeError(f"store_append: rows_out: expected [>= {capacity}, {E}] fp16 / bf16 / fp32, got "
                              f"{tuple(rows_out.shape)} {rows_out.dtype}")
        if rows_out.dtype != x.dtype and torch.float32 not in (rows_out.dtype, x.dtype):
            raise NativeError(f"store_append: {x.dtype} -> {rows_out.dtype} is not a conversion the store makes (convert the batch)",
                              _lib.MM_EUNSUPPORTED)
    if codes_out is not None:
        if (codes_out.dtype != torch.uint8 or codes_out.dim() != 2 or codes_out.shape[1] != E or codes_out.shape[0] < capacity
                or scales_out.dtype != torch.float32 or scales_out.dim() != 1 or scales_out.shape[0] < capacity):
            raise NativeError(f"store_append: codes_out / scales_out: expected [>= {capacity}, {E}] uint8 and [>= {capacity}] float32, got "
                              f"{tuple(codes_out.shape)} {codes_out.dtype} / {tuple(scales_out.shape)} {scales_out.dtype}")
    if (E * x.element_size()) % 16:
        raise NativeError(f"store_append: a row of E={E} {x.dtype} elements is not a multiple of 16 bytes", _lib.MM_EUNSUPPORTED)
    if codes_out is not None and E % 16:
        raise NativeError(f"store_append: an fp8 store needs E % 16 == 0, got E={E}", _lib.MM_EUNSUPPORTED)
    if n_docs * D >= 2 ** 31:
        raise NativeError(f"store_append: n_docs * D = {n_docs * D} rows in one batch, the limit is 2^31 - 1", _lib.MM_EUNSUPPORTED)
    if (fill.dtype != torch.int64 or fill.numel() != 1 or status.dtype != torch.int32 or status.numel() != 1
            or doc_begin.dtype != torch.int64 or doc_end.dtype != torch.int64 or tuple(doc_begin.shape) != (n_docs,)
            or tuple(doc_end.shape) != (n_docs,)):
        raise NativeError(f"store_append: fill [1] int64, status [1] int32 and doc_begin / doc_end [{n_docs}] int64 needed")
    for name, t in (("rows_out", rows_out), ("codes_out", codes_out), ("scales_out", scales_out), ("fill", fill),
                    ("doc_begin", doc_begin), ("doc_end", doc_end), ("status", status)):
        if t is not None and not t.is_contiguous():
            raise NativeError(f"store_append: {name} is written in place and must be contiguous")
    if n_docs == 0:
        return
    x = x.contiguous()
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    L = _lib.lib()
    _call(dev, L.mm_store_append, (x.data_ptr(), n_docs, D, E, _DT[x.dtype], _lib.STORE_KEEP_ZERO_ROWS if keep_zero_rows else 0,
                                   p(rows_out), _DT[rows_out.dtype] if rows_out is not None else _DT[x.dtype], p(codes_out),
                                   p(scales_out), capacity, fill.data_ptr(), doc_begin.data_ptr(), doc_end.data_ptr(),
                                   status.data_ptr()),
          L.mm_store_append_workspace_bytes, (n_docs, D), cached=True)


def _pacrr_params(weights, biases, C: int, dev):
    """Packs the conv weights ([C, 1, n, n] or [C, n, n], widths 2 .. N in order) and biases ([C] each) into the two float
    buffers of mm_pacrr_fwd: C * (4 + .. + N^2) weights, (N - 1) * C biases.  Returns (w, b) or (None, None) for N = 1."""
    weights, biases = list(weights), list(biases)
    if len(weights) != len(biases):
        raise NativeError(f"pacrr: {len(weights)} weight tensors but {len(biases)} bias tensors")
    if not weights:
        return None, None
    for i, (w, b) in enumerate(zip(weights, biases)):
        n = i + 2
        if w.numel() != C * n * n or b.numel() != C:
            raise NativeError(f"pacrr: width {n} needs weight [{C}, 1, {n}, {n}] and bias [{C}], got "
                              f"{tuple(w.shape)} / {tuple(b.shape)}")
    _dev_check(*weights, *biases)
    w = torch.cat([t.detach().reshape(-1) for t in weights]).to(device=dev, dtype=torch.float32).contiguous()
    b = torch.cat([t.detach().reshape(-1) for t in biases]).to(device=dev, dtype=torch.float32).contiguous()
    return w, b


def _pacrr_shapes(q, d, pairs_per_query, k):
    nq, Q, E, B, D = _qd_shapes(q, d, pairs_per_query)
    if not (1 <= k <= 32) or not (k <= D <= 2048) or not (1 <= Q <= 64) or E > 1024:
        # the reference's torch.topk raises for D < k (pacrr.py:86); the kernel's limits are in mm_native.h
        raise NativeError(f"pacrr_kmax: Q = {Q}, D = {D}, E = {E}, k = {k} outside 1 <= Q <= 64, k <= D <= 2048, "
                          f"E <= 1024, 1 <= k <= 32 (MM_EUNSUPPORTED)")
    return nq, Q, E, B, D


def _pacrr_fwd_setup(what, q, d, weights, biases, k, pairs_per_query, check=None):
    """What pacrr_kmax and co_pacrr_kmax share before their launch: device / dtype / shape validation (`check`: the
    model's own, on the true E), the packed parameters, E padded to a multiple of 4.
    Returns (dev, q, d, w_ptr, b_ptr, B, Q, D, E, C, N)."""
    dev = _dev_check(q, d)
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError(f"{what}: float32 embeddings only (the reference cosine rejects bf16)")
    nq, Q, E, B, D = _pacrr_shapes(q, d, pairs_per_query, k)
    if check is not None:
        check(B, Q, D, E)
    weights, biases = list(weights), list(biases)
    C = weights[0].shape[0] if weights else 1
    N = len(weights) + 1
    w, b = _pacrr_params(weights, biases, C, dev)
    if B:
        q, d, E = _pad_rows(q, d, 4)
    return (dev, q, d, w.data_ptr() if w is not None else None, b.data_ptr() if b is not None else None, B, Q, D, E, C, N)


def _pacrr_bwd(name, fn, size_fn, q, d, weights, idx, grad_out, k, pairs_per_query, idx_shape, go_shape, size_key, extra=(),
               check=None):
    """The backward both models share around their launch.  idx_shape / go_shape: (B, Q, N) -> the shapes idx / grad_out
    must have; the launch is fn(q, d, w, idx, go, gq, gd, gw, gb, B, pairs_per_query, Q, D, E, C, N, k, *extra, ..), fn =
    mm_<name>_bwd, with a workspace of size_fn(*size_key(B, Q, D, E, C, N)).  After it: E un-padded, the
    per-pair grad_q rows summed per query in group order, grad_w / grad_b summed over the pairs and split per width."""
    what = name + "_kmax_bwd"
    dev = _dev_check(q, d, idx, grad_out)
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError(f"{what}: float32 embeddings only")
    nq, Q, E0, B, D = _pacrr_shapes(q, d, pairs_per_query, k)
    if check is not None:
        check(B, Q, D, E0)
    weights = list(weights)
    C = weights[0].shape[0] if weights else 1
    N = len(weights) + 1
    w, _ = _pacrr_params(weights, [t.new_zeros(C) for t in weights], C, dev)
    if tuple(idx.shape) != idx_shape(B, Q, N) or idx.dtype != torch.int32:
        raise NativeError(f"{what}: idx must be int32 {idx_shape(B, Q, N)}, got {idx.dtype} {tuple(idx.shape)}")
    go = grad_out.detach().to(torch.float32).contiguous()
    if tuple(go.shape) != go_shape(B, Q, N):
        raise NativeError(f"{what}: grad_out must be {go_shape(B, Q, N)}, got {tuple(go.shape)}")
    idx = idx.contiguous()
    q, d, E = _pad_rows(q, d, 4)
    S = sum(n * n for n in range(2, N + 1))
    gq = torch.empty((B, Q, E), dtype=torch.float32, device=dev)
    gd = torch.empty((B, D, E), dtype=torch.float32, device=dev)
    gw = torch.empty((B, C * S), dtype=torch.float32, device=dev)
    gb = torch.empty((B, C * (N - 1)), dtype=torch.float32, device=dev)
    if B:
        ptrs = (q.data_ptr(), d.data_ptr(), w.data_ptr() if w is not None else None, idx.data_ptr(), go.data_ptr(),
                gq.data_ptr(), gd.data_ptr(), gw.data_ptr() if N > 1 else None, gb.data_ptr() if N > 1 else None)
        _call(dev, fn, ptrs + (B, pairs_per_query, Q, D, E, C, N, k) + tuple(extra), size_fn, size_key(B, Q, D, E, C, N))
    gq, gd = _trim(gq, E0), _trim(gd, E0)
    if pairs_per_query > 1:       # per-pair rows -> per query (padded to whole groups, then summed in group order)
        pad = nq * pairs_per_query - B
        if pad:
            gq = torch.cat([gq, gq.new_zeros((pad, Q, E0))])
        gq = gq.view(nq, pairs_per_query, Q, E0).sum(1)
    gw, gb = gw.sum(0), gb.sum(0)
    grad_w, grad_b, off = [], [], 0
    for i, t in enumerate(weights):
        n = i + 2
        grad_w.append(gw[C * off:C * (off + n * n)].view(t.shape).clone())     # separate tensors (no views of one sum)
        grad_b.append(gb[C * i:C * (i + 1)].clone())
        off += n * n
    return gq, gd, grad_w, grad_b


def pacrr_kmax(q: torch.Tensor, d: torch.Tensor, weights, biases, k: int, pairs_per_query: int = 1, save: bool = False):
    """PACRR's match matrix + n-gram convolutions + k-max pooling (matchmaker/models/pacrr.py:78-97) in ONE launch
    (mm_pacrr_fwd): per_query_results [n_pairs, Q, k N], paths 0, 2, .., N.

    q [n_queries, Q, E], d [n_pairs, D, E] float32; pair p scores against query p // pairs_per_query.
    weights / biases: the Conv2d parameters of widths 2 .. N (convolutions.<n-2>.1.weight [C, 1, n, n] / .bias [C]), N - 1
    of each (empty for N = 1).  save=True also returns the int32 indices [n_pairs, Q, k N] (column | channel << 16) that
    pacrr_kmax_bwd takes; the values are the same bits either way."""
    dev, q, d, w, b, B, Q, D, E, C, N = _pacrr_fwd_setup("pacrr_kmax", q, d, weights, biases, k, pairs_per_query)
    out = torch.empty((B, Q, k * N), dtype=torch.float32, device=dev)
    idx = torch.empty((B, Q, k * N), dtype=torch.int32, device=dev) if save else None
    if B:
        _call(dev, _lib.lib().mm_pacrr_fwd, (q.data_ptr(), d.data_ptr(), w, b, out.data_ptr(),
                                             idx.data_ptr() if idx is not None else None, B, pairs_per_query, Q, D, E, C, N, k))
    return (out, idx) if save else out


def pacrr_kmax_bwd(q: torch.Tensor, d: torch.Tensor, weights, idx: torch.Tensor, grad_out: torch.Tensor, k: int,
                   pairs_per_query: int = 1):
    """Backward of pacrr_kmax (mm_pacrr_bwd): idx as returned by pacrr_kmax(..., save=True) on the same inputs, grad_out
    [n_pairs, Q, k N].  Returns float32 (grad_q [n_queries, Q, E], grad_d [n_pairs, D, E], grad_w, grad_b) with grad_w /
    grad_b lists shaped like `weights` / their biases ([C]), summed over the pairs in a fixed order (no atomics)."""
    shape = lambda B, Q, N: (B, Q, k * N)
    L = _lib.lib()
    return _pacrr_bwd("pacrr", L.mm_pacrr_bwd, L.mm_pacrr_workspace_bytes, q, d, weights, idx, grad_out, k, pairs_per_query, shape, shape,
                      lambda B, Q, D, E, C, N: (B, Q, D, C, N, k))


def co_pacrr_views(unified_document_length: int):
    """The four k-max view sizes of CO-PACRR, computed as the reference does (co_pacrr.py:73-74): int(U * f)."""
    return [int(unified_document_length * x) for x in [0.25, 0.5, 0.75, 1]]


def _co_pacrr_check(B, Q, D, E, k, views):
    if len(views) != 4 or any(views[i] > views[i + 1] for i in range(3)):
        raise NativeError(f"co_pacrr_kmax: four ascending view sizes needed, got {list(views)}")
    if not (1 <= k <= 8) or not (k <= D <= 2048) or not (1 <= Q <= 64) or E > 1024 or views[0] < k:
        # the reference's torch.topk raises for a view (or D) narrower than k (co_pacrr.py:115, :140); the kernel's limits are in
        # mm_native.h
        raise NativeError(f"co_pacrr_kmax: Q = {Q}, D = {D}, E = {E}, k = {k}, views {list(views)} outside 1 <= Q <= 64, "
                          f"k <= D <= 2048, E <= 1024, 1 <= k <= 8, views >= k (MM_EUNSUPPORTED)")


def co_pacrr_kmax(q: torch.Tensor, d: torch.Tensor, weights, biases, k: int, views, pairs_per_query: int = 1,
                  save: bool = False):
    """CO-PACRR's match matrix + n-gram convolutions + k-max pooling at four views + context similarities
    (matchmaker/models/co_pacrr.py:90-158) in ONE launch (mm_co_pacrr_fwd): per_query_results [n_pairs, Q, 8 k N], per
    path 0, 2, .., N the 4k values of views 0..3 then their 4k contexts.

    q / d / weights / biases as pacrr_kmax; views: the four view sizes (co_pacrr_views(U)).  save=True also returns the
    int32 positions [n_pairs, Q, N, 4 k] (column | channel << 16) that co_pacrr_kmax_bwd takes; the values are the same
    bits either way."""
    views = [int(v) for v in views]
    dev, q, d, w, b, B, Q, D, E, C, N = _pacrr_fwd_setup("co_pacrr_kmax", q, d, weights, biases, k, pairs_per_query,
                                                         lambda B, Q, D, E: _co_pacrr_check(B, Q, D, E, k, views))
    out = torch.empty((B, Q, 8 * k * N), dtype=torch.float32, device=dev)
    idx = torch.empty((B, Q, N, 4 * k), dtype=torch.int32, device=dev) if save else None
    if B:
        _call(dev, _lib.lib().mm_co_pacrr_fwd, (q.data_ptr(), d.data_ptr(), w, b, out.data_ptr(),
                                                idx.data_ptr() if idx is not None else None, B, pairs_per_query, Q, D, E, C, N,
                                                k, *views))
    return (out, idx) if save else out


def co_pacrr_kmax_bwd(q: torch.Tensor, d: torch.Tensor, weights, idx: torch.Tensor, grad_out: torch.Tensor, k: int, views,
                      pairs_per_query: int = 1):
    """Backward of co_pacrr_kmax (mm_co_pacrr_bwd, one launch): idx as returned by co_pacrr_kmax(..., save=True) on the same
    inputs, grad_out [n_pairs, Q, 8 k N].  Returns float32 (grad_q [n_queries, Q, E], grad_d [n_pairs, D, E], grad_w,
    grad_b) as pacrr_kmax_bwd."""
    views = [int(v) for v in views]
    L = _lib.lib()
    return _pacrr_bwd("co_pacrr", L.mm_co_pacrr_bwd, L.mm_co_pacrr_workspace_bytes, q, d, weights, idx, grad_out, k, pairs_per_query,
                      lambda B, Q, N: (B, Q, N, 4 * k), lambda B, Q, N: (B, Q, 8 * k * N),
                      lambda B, Q, D, E, C, N: (B, Q, D, E, C, N, k), views,
                      lambda B, Q, D, E: _co_pacrr_check(B, Q, D, E, k, views))


# ---------------------------------------------------------------------------------------------- DRMM
def _drmm_shapes(q, d, pairs_per_query, bins, what):
    nq, Q, E, B, D = _qd_shapes(q, d, pairs_per_query)
    if not (1 <= Q <= 64) or not (1 <= D <= 65535) or E > 1024 or not (1 <= bins <= 16):
        raise NativeError(f"{what}: Q = {Q}, D = {D}, E = {E}, bins = {bins} outside 1 <= Q <= 64, 1 <= D <= 65535, "
                          f"E <= 1024, 1 <= bins <= 16 (MM_EUNSUPPORTED)")
    return nq, Q, E, B, D


def _drmm_len(d_len, B, dev):
    if d_len is None:
        return None
    t = d_len.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if t.numel() != B:
        raise NativeError(f"d_len has {t.numel()} entries for {B} pairs")
    return t


def _drmm_call(what, q, d, bins, pairs_per_query, d_len, clamp, want_hist, head):
    dev = _dev_check(q, d, d_len, *(head or ()))
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError(f"{what}: float32 embeddings only (the reference cosine rejects bf16)")
    nq, Q, E, B, D = _drmm_shapes(q, d, pairs_per_query, bins, what)
    dl = _drmm_len(d_len, B, dev)
    hist = torch.empty((B, Q, bins), dtype=torch.float32, device=dev) if want_hist else None
    score = gate = W1 = b1 = w2 = b2 = None
    per_pair = 0
    if head is not None:
        gate, W1, b1, w2, b2 = head
        gate = gate.detach().to(torch.float32).contiguous()
        if tuple(gate.shape) == (B, Q) and B != nq:
            per_pair = 1
        elif tuple(gate.shape) != (nq, Q):
            raise NativeError(f"{what}: gate must be {(nq, Q)} (per query) or {(B, Q)} (per pair), got {tuple(gate.shape)}")
        W1, b1, w2, b2 = _vec(W1.detach()), _vec(b1.detach()), _vec(w2.detach()), _vec(b2.detach())
        if W1.numel() != bins * bins or b1.numel() != bins or w2.numel() != bins or b2.numel() != 1:
            raise NativeError(f"{what}: head parameters must be W1 [{bins}, {bins}], b1 [{bins}], w2 [{bins}], b2 [1]")
        score = torch.empty(B, dtype=torch.float32, device=dev)
    if B:
        q, d, E = _pad_rows(q, d, 4)
        p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        _call(dev, _lib.lib().mm_drmm_fwd, (q.data_ptr(), d.data_ptr(), p(dl), p(hist), p(score), p(gate), per_pair, p(W1),
                                            p(b1), p(w2), p(b2), B, pairs_per_query, Q, D, E, bins, 1 if clamp else 0))
    return hist, score


def drmm_hist(q: torch.Tensor, d: torch.Tensor, bins: int = 10, pairs_per_query: int = 1,
              d_len: Optional[torch.Tensor] = None, clamp: bool = False) -> torch.Tensor:
    """DRMM's matching histograms (matchmaker/models/drmm.py:66-74) in ONE launch (mm_drmm_fwd), nothing leaves the device:
    hist [n_pairs, Q, bins] float32 = torch.histc(cosine(q_i, d)[i, :], bins, -1, 1) per query token (raw counts; cosines
    that round above 1 are dropped, as histc drops them; clamp=True clamps them into the last bin instead — a deviation).

    q [n_queries, Q, E], d [n_pairs, D, E] float32 with padding / OOV rows already multiplied to zero (:56-58); pair p
    scores against query p // pairs_per_query.  d_len [n_pairs] (optional): rows at or past it are zero rows and are not
    read (bit-equal to reading them).  No gradient flows through a histogram."""
    return _drmm_call("drmm_hist", q, d, bins, pairs_per_query, d_len, clamp, True, None)[0]


def drmm_score(q: torch.Tensor, d: torch.Tensor, gate: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
               b2: torch.Tensor, pairs_per_query: int = 1, d_len: Optional[torch.Tensor] = None, clamp: bool = False,
               return_hist: bool = False):
    """DRMM's score with the head fused into the histogram kernel (inference; drmm.py:66-91): score [n_pairs] =
    sum_i gate[., i] * tanh(w2 . tanh(W1 log1p(hist_i) + b1) + b2).  gate [n_queries, Q] or [n_pairs, Q]: the masked
    softmax of the query gate, computed by the caller; W1 [bins, bins], b1 [bins], w2 [bins] (or [1, bins]), b2 [1] =
    matching_classifier._linear_layers.{0,1}.{weight,bias}.  return_hist=True also returns the histograms of the same
    launch (the same bits as drmm_hist)."""
    bins = b1.numel()
    hist, score = _drmm_call("drmm_score", q, d, bins, pairs_per_query, d_len, clamp, return_hist, (gate, W1, b1, w2, b2))
    return (score, hist) if return_hist else score


# ---------------------------------------------------------------------------------------------- MatchPyramid
def _mp_layers(Q, D, weights, biases, pool_sizes, what):
    """-> (host int32 array [L, 5] of (C, k0, k1, ph, pw), feature count).  Only the consistency of the lists is checked
    here; the envelope is mm_matchpyramid_fwd's to judge (MM_EUNSUPPORTED before any launch)."""
    L = len(weights)
    if L < 1 or len(biases) != L or len(pool_sizes) != L:
        raise NativeError(f"{what}: {L} weights, {len(biases)} biases, {len(pool_sizes)} pool sizes")
    rows, cin = [], 1
    for wt, bs, pool in zip(weights, biases, pool_sizes):
        if wt.dim() != 4 or wt.shape[1] != cin or bs.numel() != wt.shape[0]:
            raise NativeError(f"{what}: conv weight {tuple(wt.shape)} / bias {tuple(bs.shape)} after {cin} channels")
        cin = int(wt.shape[0])
        rows.append((cin, int(wt.shape[2]), int(wt.shape[3]), int(pool[0]), int(pool[1])))
    return (ctypes.c_int32 * (5 * L))(*[x for r in rows for x in r]), max(cin * rows[-1][3] * rows[-1][4], 0)


def mm_matchpyramid_workspace_bytes(B, Q, D, L, *layers):
    """The size query on integers alone (the layer table flattened), so that _ws_bytes can key it like the others."""
    return _lib.lib().mm_matchpyramid_workspace_bytes(B, Q, D, L, (ctypes.c_int32 * len(layers))(*layers))


def matchpyramid_pack(weights, biases):
    """The conv weights / biases of every layer in mm_matchpyramid_fwd's packing (two float32 vectors)."""
    w = torch.cat([t.detach().to(torch.float32).reshape(-1) for t in weights])
    b = torch.cat([t.detach().to(torch.float32).reshape(-1) for t in biases])
    return w, b


def matchpyramid_features(q: torch.Tensor, d: torch.Tensor, weights, biases, pool_sizes, pairs_per_query: int = 1,
                          packed=None) -> torch.Tensor:
    """MatchPyramid's forward up to the flattened conv result (matchmaker/models/matchpyramid.py:74-92) in ONE launch
    (mm_matchpyramid_fwd): features [n_pairs, C_L ph_L pw_L] float32, channel-major as `.view(B, -1)` gives.

    q [n_queries, Q, E], d [n_pairs, D, E] float32 (no mask enters, as in the reference); pair p scores against query
    p // pairs_per_query.  weights[l] [C_l, C_{l-1}, k0, k1], biases[l] [C_l], pool_sizes[l] (ph, pw).  packed (optional):
    matchpyramid_pack(weights, biases) made earlier.  Inference only.  Raises NativeError whose .code is the C return code
    (MM_EUNSUPPORTED outside the envelope, before any launch)."""
    dev = _dev_check(q, d, *weights, *biases)
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError("matchpyramid_features: float32 embeddings only (the reference cosine rejects bf16)")
    nq, Q, E, B, D = _qd_shapes(q, d, pairs_per_query)
    layers, feat = _mp_layers(Q, D, weights, biases, pool_sizes, "matchpyramid_features")
    out = torch.empty((B, feat), dtype=torch.float32, device=dev)
    if B:
        w, b = packed if packed is not None else matchpyramid_pack(weights, biases)
        q, d, E = _pad_rows(q, d, 4)
        L = len(weights)
        _call(dev, _lib.lib().mm_matchpyramid_fwd, (q.data_ptr(), d.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), B,
                                                    pairs_per_query, Q, D, E, L, layers),
              mm_matchpyramid_workspace_bytes, (B, Q, D, L, *layers))
    return out


def mm_matchpyramid_fwd_save_workspace_bytes(B, Q, D, L, *layers):
    return _lib.lib().mm_matchpyramid_fwd_save_workspace_bytes(B, Q, D, L, (ctypes.c_int32 * len(layers))(*layers))


def mm_matchpyramid_bwd_workspace_bytes(B, Q, D, L, *layers):
    return _lib.lib().mm_matchpyramid_bwd_workspace_bytes(B, Q, D, L, (ctypes.c_int32 * len(layers))(*layers))


def matchpyramid_saved_size(weights, pool_sizes) -> int:
    """S = sum_l C_l ph_l pw_l: the pooled elements of one pair over all layers (the row length of the saved state)."""
    return sum(int(w.shape[0]) * int(p[0]) * int(p[1]) for w, p in zip(weights, pool_sizes))


def matchpyramid_features_save(q: torch.Tensor, d: torch.Tensor, weights, biases, pool_sizes, pairs_per_query: int = 1,
                               packed=None):
    """matchpyramid_features for training (mm_matchpyramid_fwd_save): -> (features, saved), features the same bits as
    matchpyramid_features, saved = (pooled [n_pairs, S] float32, argmax [n_pairs, S] int32), S = sum_l C_l ph_l pw_l: per
    pair, layer after layer, every layer's pooled output [C_l, ph_l, pw_l] and for each of its elements the flat index
    row * Wo + col into the channel's conv output (F.adaptive_max_pool2d(return_indices=True)'s convention; among equal
    maxima the first in row-major order).  matchpyramid_bwd takes `saved`."""
    dev = _dev_check(q, d, *weights, *biases)
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError("matchpyramid_features_save: float32 embeddings only (the reference cosine rejects bf16)")
    nq, Q, E, B, D = _qd_shapes(q, d, pairs_per_query)
    layers, feat = _mp_layers(Q, D, weights, biases, pool_sizes, "matchpyramid_features_save")
    S = matchpyramid_saved_size(weights, pool_sizes)
    out = torch.empty((B, feat), dtype=torch.float32, device=dev)
    pooled = torch.empty((B, S), dtype=torch.float32, device=dev)
    argmax = torch.empty((B, S), dtype=torch.int32, device=dev)
    if B:
        w, b = packed if packed is not None else matchpyramid_pack(weights, biases)
        q, d, E = _pad_rows(q, d, 4)
        L = len(weights)
        _call(dev, _lib.lib().mm_matchpyramid_fwd_save, (q.data_ptr(), d.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                         pooled.data_ptr(), argmax.data_ptr(), B, pairs_per_query, Q, D, E, L,
                                                         layers),
              mm_matchpyramid_fwd_save_workspace_bytes, (B, Q, D, L, *layers))
    return out, (pooled, argmax)


def matchpyramid_bwd(q: torch.Tensor, d: torch.Tensor, weights, biases, pool_sizes, saved, grad_features: torch.Tensor,
                     pairs_per_query: int = 1, packed=None):
    """Backward of matchpyramid_features_save (mm_matchpyramid_bwd): saved as returned by it on the same inputs,
    grad_features [n_pairs, C_L ph_L pw_L].  Returns float32 (grad_q [n_queries, Q, E], grad_d [n_pairs, D, E], grad_w,
    grad_b), the lists shaped like `weights` / `biases`, summed over the pairs in a fixed order (no atomics: two calls give
    the same bits).  For pairs_per_query > 1 the per-pair grad_q rows of a query are summed here, in pair order."""
    pooled, argmax = saved
    dev = _dev_check(q, d, pooled, argmax, grad_features, *weights, *biases)
    q, d = _emb(q, "q"), _emb(d, "d")
    if q.dtype != torch.float32 or d.dtype != torch.float32:
        raise NativeError("matchpyramid_bwd: float32 embeddings only")
    nq, Q, E0, B, D = _qd_shapes(q, d, pairs_per_query)
    layers, feat = _mp_layers(Q, D, weights, biases, pool_sizes, "matchpyramid_bwd")
    S = matchpyramid_saved_size(weights, pool_sizes)
    if tuple(pooled.shape) != (B, S) or pooled.dtype != torch.float32 or tuple(argmax.shape) != (B, S) \
            or argmax.dtype != torch.int32:
        raise NativeError(f"matchpyramid_bwd: saved must be (float32, int32) [{B}, {S}], got {pooled.dtype} "
                          f"{tuple(pooled.shape)}, {argmax.dtype} {tuple(argmax.shape)}")
    go = grad_features.detach().to(torch.float32).contiguous()
    if tuple(go.shape) != (B, feat):
        raise NativeError(f"matchpyramid_bwd: grad_features must be [{B}, {feat}], got {tuple(go.shape)}")
    pooled, argmax = pooled.contiguous(), argmax.contiguous()
    w, _ = packed if packed is not None else matchpyramid_pack(weights, biases)
    q, d, E = _pad_rows(q, d, 4)
    gq = torch.empty((B, Q, E), dtype=torch.float32, device=dev)
    gd = torch.empty((B, D, E), dtype=torch.float32, device=dev)
    gw = torch.zeros(w.numel(), dtype=torch.float32, device=dev)
    gb = torch.zeros(sum(int(t.shape[0]) for t in weights), dtype=torch.float32, device=dev)
    if B:
        L = len(weights)
        _call(dev, _lib.lib().mm_matchpyramid_bwd, (q.data_ptr(), d.data_ptr(), w.data_ptr(), pooled.data_ptr(), argmax.data_ptr(),
                                                    go.data_ptr(), gq.data_ptr(), gd.data_ptr(), gw.data_ptr(), gb.data_ptr(), B,
                                                    pairs_per_query, Q, D, E, L, layers),
              mm_matchpyramid_bwd_workspace_bytes, (B, Q, D, L, *layers))
    gq, gd = _trim(gq, E0), _trim(gd, E0)
    if pairs_per_query > 1:       # per-pair rows -> per query (padded to whole groups, then summed in group order)
        pad = nq * pairs_per_query - B
        if pad:
            gq = torch.cat([gq, gq.new_zeros((pad, Q, E0))])
        gq = gq.view(nq, pairs_per_query, Q, E0).sum(1)
    grad_w, grad_b, wo, bo = [], [], 0, 0
    for t, bs in zip(weights, biases):
        grad_w.append(gw[wo:wo + t.numel()].view(t.shape).clone())     # separate tensors (no views of one buffer)
        grad_b.append(gb[bo:bo + t.shape[0]].view(bs.shape).clone())
        wo += t.numel()
        bo += int(t.shape[0])
    return gq, gd, grad_w, grad_b


# ---- ranking and IR metrics (rank_metrics.hip) --------------------------------------------------------------------------
RANK_MAX_LEN = _lib.RANK_MAX_LEN            # rows per segment of segment_rank, thresholds of rank_metrics_depth
RANK_NOT_JUDGED = _lib.RANK_NOT_JUDGED      # grade of a row whose document is not in its query's qrels


def _seg_begin_check(op: str, seg_begin: torch.Tensor):
    if seg_begin.dim() != 1 or seg_begin.dtype != torch.int64 or seg_begin.shape[0] < 1:
        raise NativeError(f"{op}: seg_begin must be int64 [nq + 1], got {seg_begin.dtype} {tuple(seg_begin.shape)}")


def segment_rank(scores: torch.Tensor, seg_begin: torch.Tensor, max_len: int) -> torch.Tensor:
    """Per-query rank order of flat scores (utils/core_metrics.py:502-511; native mm_segment_rank_fwd).

    scores [N] float32 / float16 / bfloat16 in arrival order; seg_begin [nq + 1] int64, ascending: query s owns rows
    [seg_begin[s], seg_begin[s + 1]); max_len >= every segment length, at most RANK_MAX_LEN (more is refused: the caller
    takes another route).  Returns order [N] int32: order[seg_begin[s] + r] is the row with rank r + 1 in query s — higher
    score first, equal scores in arrival order, -0.0 == +0.0, NaN after everything else.  One or two launches on the current
    stream, no workspace, no read-back: graph-capturable."""
    dev = _dev_check(scores, seg_begin)
    if scores.dim() != 1 or scores.dtype not in _DT:
        raise NativeError(f"segment_rank: scores must be float32 / float16 / bfloat16 [N], got {scores.dtype} {tuple(scores.shape)}")
    _seg_begin_check("segment_rank", seg_begin)
    max_len = int(max_len)
    if not 0 <= max_len <= RANK_MAX_LEN:
        raise NativeError(f"segment_rank: max_len={max_len} outside 0 .. {RANK_MAX_LEN} rows per segment", _lib.MM_EUNSUPPORTED)
    n, nq = scores.shape[0], seg_begin.shape[0] - 1
    if n >= 1 << 31:
        raise NativeError(f"segment_rank: n={n} >= 2^31", _lib.MM_EUNSUPPORTED)
    scores, seg_begin = scores.contiguous(), seg_begin.contiguous()
    order = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0 or nq == 0:
        return order
    _call(dev, _lib.lib().mm_segment_rank_fwd, (scores.data_ptr(), _DT[scores.dtype], seg_begin.data_ptr(), n, nq, max_len,
                                                order.data_ptr()), stream_only=True)
    return order


def _cutoffs(op: str, name: str, cutoffs):
    cutoffs = [int(c) for c in cutoffs]
    if len(cutoffs) > _lib.RANK_MAX_CUTOFFS or any(c < 1 for c in cutoffs):
        raise NativeError(f"{op}: {name}={cutoffs}: at most {_lib.RANK_MAX_CUTOFFS} cutoffs, each >= 1", _lib.MM_EUNSUPPORTED)
    return cutoffs, (ctypes.c_int32 * max(len(cutoffs), 1))(*cutoffs)


def _rank_metrics(op, fn, per_query, order, seg_begin, grade, cand_pos, scalar, binarization_point, mrr_cutoffs, ndcg_cutoffs,
                  map_cutoff, binary_num_relevant, idcg, log2_table):
    """The checks and the call rank_metrics and rank_metrics_depth share; per_query = output entries per query (1 / hi)."""
    dev = _dev_check(order, seg_begin, grade, cand_pos, binary_num_relevant, idcg, log2_table)
    _seg_begin_check(op, seg_begin)
    n, nq = order.shape[0], seg_begin.shape[0] - 1
    rows = [("order", order), ("grade", grade)] + ([("cand_pos", cand_pos)] if cand_pos is not None else [])
    for name, t in rows:
        if t.dim() != 1 or t.dtype != torch.int32 or t.shape[0] != n:
            raise NativeError(f"{op}: {name} must be int32 [{n}], got {t.dtype} {tuple(t.shape)}")
    rc, rc_c = _cutoffs(op, "mrr_cutoffs", mrr_cutoffs)
    nc, nc_c = _cutoffs(op, "ndcg_cutoffs", ndcg_cutoffs)
    if int(map_cutoff) < 1:
        raise NativeError(f"{op}: map_cutoff={map_cutoff} below 1")
    if binary_num_relevant.dtype != torch.int32 or tuple(binary_num_relevant.shape) != (nq,):
        raise NativeError(f"{op}: binary_num_relevant must be int32 [{nq}], got {binary_num_relevant.dtype} "
                          f"{tuple(binary_num_relevant.shape)}")
    if idcg.dtype != torch.float64 or tuple(idcg.shape) != (nq, len(nc)):
        raise NativeError(f"{op}: idcg must be float64 [{nq}, {len(nc)}], got {idcg.dtype} {tuple(idcg.shape)}")
    if log2_table.dtype != torch.float64 or log2_table.dim() != 1 or log2_table.shape[0] <= max(nc, default=0):
        raise NativeError(f"{op}: log2_table must be float64 [> {max(nc, default=0)}] (log2(1 + r) up to the largest nDCG cutoff), "
                          f"got {log2_table.dtype} {tuple(log2_table.shape)}")
    if n >= 1 << 31:
        raise NativeError(f"{op}: n={n} >= 2^31", _lib.MM_EUNSUPPORTED)
    order, seg_begin, grade = order.contiguous(), seg_begin.contiguous(), grade.contiguous()
    cand_pos = cand_pos.contiguous() if cand_pos is not None else None
    binary_num_relevant, idcg, log2_table = binary_num_relevant.contiguous(), idcg.contiguous(), log2_table.contiguous()
    shape = (nq,) if per_query is None else (nq, per_query)
    first_rank = torch.empty(shape, dtype=torch.int32, device=dev)
    hits = torch.empty(shape + (len(rc),), dtype=torch.int32, device=dev)
    ap = torch.empty(shape, dtype=torch.float64, device=dev)
    ndcg = torch.empty(shape + (len(nc),), dtype=torch.float64, device=dev)
    if nq:
        _call(dev, fn, (order.data_ptr() if n else None, seg_begin.data_ptr(), grade.data_ptr() if n else None,
                        cand_pos.data_ptr() if cand_pos is not None and n else None, n, nq, int(scalar), float(binarization_point),
                        ctypes.addressof(rc_c), len(rc), ctypes.addressof(nc_c), len(nc), int(map_cutoff),
                        binary_num_relevant.data_ptr(), idcg.data_ptr(), log2_table.data_ptr(), log2_table.shape[0],
                        first_rank.data_ptr(), hits.data_ptr() if rc else None, ap.data_ptr(), ndcg.data_ptr() if nc else None),
              stream_only=True)
    return first_rank, hits, ap, ndcg


def rank_metrics(order: torch.Tensor, seg_begin: torch.Tensor, grade: torch.Tensor, cand_pos: Optional[torch.Tensor],
                 threshold: int, binarization_point: float, mrr_cutoffs, ndcg_cutoffs, map_cutoff: int,
                 binary_num_relevant: torch.Tensor, idcg: torch.Tensor, log2_table: torch.Tensor):
    """Per-query metric quantities at one candidate threshold (the per-query bodies of calculate_metrics_plain,
    utils/core_metrics.py:380-461, and calculate_metrics_single_candidate_threshold, :228-327; native mm_rank_metrics_fwd).

    order [N] int32 (segment_rank's), grade [N] int32 (RANK_NOT_JUDGED = not in the query's qrels), cand_pos [N] int32 or
    None; rows with cand_pos > threshold are dropped and the rest renumbered (threshold = 2^31-1 with cand_pos None is the
    plain form).  binary_num_relevant [nq] int32, idcg [nq, len(ndcg_cutoffs)] float64, log2_table float64 = log2(1 + r).
    Returns (first_rank [nq] int32, hits [nq, len(mrr_cutoffs)] int32, ap [nq] float64, ndcg [nq, len(ndcg_cutoffs)]
    float64).  One launch on the current stream, no workspace, no atomics: graph-capturable, bit-equal run to run."""
    if not -2 ** 31 <= int(threshold) < 2 ** 31:
        raise NativeError(f"rank_metrics: threshold={threshold} is not an int32")
    return _rank_metrics("rank_metrics", _lib.lib().mm_rank_metrics_fwd, None, order, seg_begin, grade, cand_pos, threshold,
                         binarization_point, mrr_cutoffs, ndcg_cutoffs, map_cutoff, binary_num_relevant, idcg, log2_table)


def rank_metrics_depth(order: torch.Tensor, seg_begin: torch.Tensor, grade: torch.Tensor, cand_pos: torch.Tensor, hi: int,
                       binarization_point: float, mrr_cutoffs, ndcg_cutoffs, map_cutoff: int,
                       binary_num_relevant: torch.Tensor, idcg: torch.Tensor, log2_table: torch.Tensor):
    """rank_metrics at every candidate threshold t = 1 .. hi in one launch (calculate_metrics_along_candidate_depth,
    utils/core_metrics.py:42-173, without its [hi, hi] mask; native mm_rank_metrics_depth_fwd).  hi <= RANK_MAX_LEN; every
    segment must be at most hi rows long (the caller checks: the reference raises there).  Returns (first_rank [nq, hi],
    hits [nq, hi, nR], ap [nq, hi], ndcg [nq, hi, nN]); entry t - 1 is rank_metrics(threshold=t)."""
    hi = int(hi)
    if cand_pos is None:
        raise NativeError("rank_metrics_depth: cand_pos is needed (the sweep is over first-stage ranks)")
    if not 1 <= hi <= RANK_MAX_LEN:
        raise NativeError(f"rank_metrics_depth: hi={hi} outside 1 .. {RANK_MAX_LEN} thresholds", _lib.MM_EUNSUPPORTED)
    return _rank_metrics("rank_metrics_depth", _lib.lib().mm_rank_metrics_depth_fwd, hi, order, seg_begin, grade, cand_pos, hi,
                         binarization_point, mrr_cutoffs, ndcg_cutoffs, map_cutoff, binary_num_relevant, idcg, log2_table)
