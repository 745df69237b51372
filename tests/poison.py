"""Poisoned-memory harness (a helper like tests/abi.py, not a test module): while it is active, every `torch.empty` of
matchmaker_amd/ops.py and every workspace comes out of an arena filled with a poison byte, 256-byte aligned, with a guard band
of the same byte on each side.  After the call the harness says whether every guard byte is still the poison (an overrun
corrupts a canary inside an allocated tensor: nothing faults) and hands the outputs back as integer views, so that two runs
under two different poisons can be compared bit for bit — an element the operator did not write, or computed from memory it did
not initialise, differs between them.

  0xFF: NaN in f64 / f32 / bf16 / f16, -1 in every integer type
  0x7F: 3.39e38 (finite) in f32 / bf16, NaN in f16, a large positive value in every integer type

Only `torch.empty` as ops.py sees it is replaced (a proxy object stands in for the module's `torch`; every other attribute is
forwarded) and `ops._workspace`, which here returns exactly the requested bytes instead of a cached max(nbytes, 65536) buffer —
so a *_workspace_bytes that is short shows as a broken guard.  `torch.zeros` stays: those allocations are deliberate
accumulators.  The same code runs on CPU tensors (tests/test_poison_harness_cpu.py).

Audit: who initialises what (read from matchmaker_amd/csrc; "W" = workspace, sizes from the entry point's *_workspace_bytes)
===============================================================================================================================
The six hipMemsetAsync calls of csrc/: tkl_bwd.hip (grad_chunks, every call with P > 0), dot_topk.hip and dot_topk_fp8.hip (the
per-query candidate counters in W), ivf_device.h (the per-list count | fill block of W, once per round) and the two of
maxsim_inbatch_bwd.hip, which serve the Bq == 0 / Bd == 0 call only (a gradient with elements but no pair is all zeros).
Everything else is written by a kernel before it is read.  Dense masks of every scoring operator are packed into W by
pack_mask_kernel / pack_mask2_kernel (common.hip): one length per row and ceil(L / 32) words per row, every one of them stored;
the bytes that round a block up to 256 are never read.  Length masks and int64 masks the kernel reads itself use no W.
The atomics of csrc/ (dot_topk.hip, dot_topk_fp8.hip, ivf_device.h, graph_search.hip, and atomicOr on LDS bit sets in maxsim.hip
and tkl_bwd.hip) touch int32 counters, histogram bins, slots and bit sets only, never a float: every operator is bit-reproducible.

entry point                    outputs: who writes which part                                W regions: initialiser
mm_maxsim_fwd, _inbatch_fwd,   out: one store per pair (a fully masked document: -1000 per   packed masks: pack kernel
mm_maxsim_ragged(_fp8)_fwd     live query token; a masked query token: 0)
mm_maxsim_bwd                  grad_q, grad_d [B, Q | D, E]: every row stored by the pair's  packed masks: pack kernel (the arg-max
                               workgroup, zeros for masked rows and for rows no arg-max      table and the row bit sets live in LDS)
mm_maxsim_inbatch_bwd          grad_q, grad_d: every element stored by the q pass / the d    packed masks: pack kernel; int16 arg-max
                               pass (LDS accumulators, zeroed per tile); a NULL one: no      table [Bq, Bd, Q]: the table pass, before
                               pass                                                          both
mm_fp8_quantize_rows           codes, scales: header "every output byte is written"          none
mm_kernel_pool_ex_fwd2         out [B], per_kernel [B, K]: one store per pair / (pair, k);   packed masks: pack kernel (none on the
                               pooled [B, Q, K]: live query rows; header "Rows of padded /   inline-mask path)
                               masked query tokens are unspecified"
mm_kernel_pool_multi_fwd       out [B]: kp_sum_blocks_kernel, one store per pair             packed masks; partial [n_q n_d, B]: one
                                                                                             store per (combination, pair) by the pooling
                                                                                             kernel before the sum reads it
mm_kernel_pool_ex_bwd2         grad_q, grad_d: split kernel (Q <= 32, K = 11, E <= 320;      packed masks; pooled sums [B, Q, K] when the
                               S workgroups per pair + combine), tiled exact-f32 kernel      caller passes none: pooling pre-pass; partial
                               (Q <= 32, E <= 512) or per-element kernel: each stores zeros  grad_q [B, S, Q E + 96] (<= 128 pairs): every
                               for masked rows; grad_alpha / grad_w [B, K] and grad_gate:    share stored by its workgroup before the
                               torch.zeros by the caller, one row per pair stored            combine kernel reads it
mm_tkl_fwd_peaks               win [B, W]: every window stored (0 without a live chunk: an   slot map [B C]: -1 by tkl_prep_kernel, then
                               empty document is a row of zeros); out [B], peaks [B, 3]:     stage 1; pair sums / cosines: stage 1, read
                               tkl_region_kernel, one workgroup per document                 through the slot map only; packed chunk and
                                                                                             query masks, emb, live tile counts: prep
                                                                                             kernel; token-group planes: window kernel
mm_tkl_bwd                     grad_chunks [P, 50, E]: hipMemsetAsync, then accumulated;     slot map: -1 by tkl_bwd_fill_kernel, then the
                               grad_q [B, Q, E], grad_params [B, NP]: stored per document    slot kernel; region flags [B, 3] (three
                               (three-workgroup form: tkl_bwd_combine_kernel adds the        workgroups per document): 0 by the fill
                               shares)                                                       kernel; shares of grad_q / grad_params:
                                                                                             stored whole by each region's workgroup
mm_dot_topk_fwd / _fp8_fwd     scores, rows [nq, k]: topk_rows_kernel stores all k           sample scores, tau: sample / fill kernels;
                               (-inf / -1 behind the survivors); status [nq]: one store      counters: hipMemsetAsync; candidate lists:
                                                                                             read below min(counter, cap) only
mm_ivf_scan_fwd / _fp8_fwd,    scores, rows [nq, k]: ivf_select_kernel stores all k of       seg_off, total: rows kernel; tstart, blk_list:
mm_ah_scan_fwd                 every query (-inf / -1 behind the union)                      tasks kernel; prefix, qbeg: chunks kernel;
                                                                                             cnt | fill: memset per round; start: list
                                                                                             scan; pairs: fill pass; cand: score kernel
mm_ah_encode, mm_gather_dot,   one store per output element (gather_dot: -inf for row -1)    none
mm_kmeans_assign
mm_kmeans_segment_sum          sums [nlist, E]: a one-chunk list by its chunk, every other   tstart: tasks kernel; partial [chunks, E]:
                               (empty ones: zeros) by kms_combine_kernel                     one row per chunk of a multi-chunk list
mm_graph_search_fwd            scores, rows [nq, k]: all k stored (-inf / -1 behind the      visited table (when not in LDS): -1 by the
                               rows reached); stats [nq, 2]                                  query's workgroup before every query
mm_topk_merge                  scores, ids [nq, k]: all k stored (-inf / -1 padding)         none
mm_colbert_candidates          cand_doc (-1), cand_begin / cand_end ((0, 0)): all c_cap      sort keys and distinct documents of the
                               slots of every query; count [nq]                              workgroup's slot: written per query
mm_store_append                in place: store rows fill .. fill + kept, doc_begin /         row flags (every 16-bit quarter of every
                               doc_end [n_docs], fill, status; rows past the new fill and    word): count kernel; prefix, ctrl: scan kernel
                               a refused batch: nothing (header)
mm_pacrr_fwd / mm_co_pacrr_fwd out, idx: every (pair, query token, slot)                     none
mm_pacrr_bwd / mm_co_pacrr_bwd grad_q, grad_d [B, ...] and the per-pair rows of grad_w /     per-pair scratch (tap sums; CO-PACRR: the
                               grad_b: every element stored by the pair's workgroup          context gradient): written by the pair's
                                                                                             workgroup before it is read
mm_drmm_fwd                    hist [B, Q, bins], score [B]: every element                   none
mm_matchpyramid_fwd(_save)     features, pooled, argmax [B, S]: every element                layer planes with their zero frames: written
                                                                                             layer by layer
mm_matchpyramid_bwd            grad_q, grad_d: every element; grad_w, grad_b: the reduce     per-workgroup weight partials: zeroed by the
                               kernel stores every element (the caller's torch.zeros is      workgroup first; gradient planes: zero frame
                               not relied on)                                                and body written before the products
mm_segment_rank_fwd            order [N]: every row of every segment (segments tile [0, N))  none
mm_rank_metrics(_depth)_fwd    first_rank, hits, ap, ndcg: one store per (query[, t])        none
"""
import contextlib
from collections import namedtuple

import pytest
import torch

GUARD = 4096            # bytes of poison on each side of every allocation
ALIGN = 256
POISONS = (0xFF, 0x7F)

Allocation = namedtuple("Allocation", "buffer offset nbytes dtype shape")

_INT_VIEW = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}


class Arena:
    """Hands out poisoned allocations and remembers them: (buffer, offset, nbytes, dtype, shape) each."""

    def __init__(self, poison: int):
        assert 0 <= poison <= 255
        self.poison = poison
        self.allocations = []

    def empty(self, *size, dtype=None, device=None, **kw):
        """torch.empty's call forms as ops.py uses them: empty(n, ...), empty((a, b), ...), empty(a, b, ...)."""
        assert not kw, f"poison arena: torch.empty keyword(s) {sorted(kw)} are not modelled"
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        shape = tuple(int(s) for s in size)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        total = GUARD + ALIGN + -(-nbytes // ALIGN) * ALIGN + GUARD
        buf = torch.full((total,), self.poison, dtype=torch.uint8, device=device)
        off = GUARD + (-(buf.data_ptr() + GUARD)) % ALIGN
        t = buf[off:off + nbytes].view(dtype).view(shape)
        assert t.data_ptr() % ALIGN == 0 and off >= GUARD and total - (off + nbytes) >= GUARD
        self.allocations.append(Allocation(buf, off, nbytes, dtype, shape))
        return t

    def broken_guards(self):
        """One line per allocation with a guard byte that is no longer the poison (empty list: every guard is intact)."""
        bad = []
        for i, a in enumerate(self.allocations):
            host = a.buffer.cpu()
            for side, band, base in (("before", host[:a.offset], -a.offset), ("after", host[a.offset + a.nbytes:], 0)):
                hit = torch.nonzero(band != self.poison).flatten()
                if hit.numel():
                    first, last = int(hit[0]) + base, int(hit[-1]) + base
                    where = f"byte {first} .. {last} relative to its {'start' if side == 'before' else 'end'}"
                    bad.append(f"allocation {i} ({a.dtype} {a.shape}, {a.nbytes} bytes): {hit.numel()} guard byte(s) {side} it "
                               f"overwritten ({where})")
        return bad

    def assert_guards_intact(self, label=""):
        bad = self.broken_guards()
        assert not bad, f"{label}: writes outside an allocation under poison {self.poison:#04x}:\n" + "\n".join(bad)


class _TorchProxy:
    """`torch` as the patched module sees it: `empty` comes from the arena, everything else is torch's own."""

    def __init__(self, arena):
        self.empty = arena.empty

    def __getattr__(self, name):
        return getattr(torch, name)


@contextlib.contextmanager
def poisoned(poison: int, module=None):
    """with poisoned(0xFF) as arena: ...one operator call...  `module` (default matchmaker_amd.ops) gets the proxy as its
    `torch` and an exact-size `_workspace`; its cached workspaces are dropped on entry and on exit.  The device is synchronised
    before the context ends, so the arena can be inspected right after."""
    if module is None:
        from matchmaker_amd import ops as module
    arena = Arena(poison)

    def _workspace(dev, nbytes, stream=None):
        return arena.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None

    module.clear_workspaces()
    try:
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(module, "torch", _TorchProxy(arena))
            mp.setattr(module, "_workspace", _workspace)
            yield arena
            if torch.cuda.is_available():
                torch.cuda.synchronize()
    finally:
        module.clear_workspaces()


def bits(t):
    """A tensor as a host integer view of its bits (NaN meets NaN); None and non-tensors pass through."""
    if not isinstance(t, torch.Tensor):
        return t
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t.view(_INT_VIEW[t.element_size()])


def flatten(out):
    """The tensors of an operator's result (a tensor, or nested tuples / lists with Nones), in order."""
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flatten(o)]
    return []


def run(fn, poison: int, module=None, label=""):
    """fn() under `poison`; asserts every guard intact; returns (result, arena)."""
    with poisoned(poison, module) as arena:
        out = fn()
    arena.assert_guards_intact(label)
    return out, arena


def assert_same_bits(a, b, label="", keep=None):
    """Two results of one operator under two poisons, tensor by tensor: bit-identical (over keep[i] where given: a boolean
    tensor, broadcastable, of the elements the header specifies)."""
    fa, fb = flatten(a), flatten(b)
    assert len(fa) == len(fb), f"{label}: {len(fa)} vs {len(fb)} output tensors"
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and x.dtype == y.dtype, f"{label}: output {i} {x.dtype} {tuple(x.shape)} vs {y.dtype} {tuple(y.shape)}"
        bx, by = bits(x), bits(y)
        diff = bx != by
        if keep is not None and keep[i] is not None:
            diff = diff & keep[i].cpu().expand_as(diff)
        n = int(diff.sum())
        if n:
            first = [int(v) for v in torch.nonzero(diff)[0]]
            raise AssertionError(f"{label}: output {i} ({x.dtype} {tuple(x.shape)}) differs between the two poisons in {n} of "
                                 f"{diff.numel()} elements, first at {first}: an element that was not written, or one computed "
                                 f"from uninitialised memory")


def poison_survivors(t, poison: int):
    """Number of elements of `t` whose every byte is still the poison byte."""
    b = t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).reshape(-1, t.element_size())
    return int((b == poison).all(dim=1).sum())
