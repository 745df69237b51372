"""Exact-arithmetic MaxSim cases: inputs on which the float64 restatement is the ONE right answer, bit for bit, with rows planted at
the positions where kernels go wrong, and a Python restatement of the dispatch that shows which kernel every case reaches.
CPU only (numpy); tests/test_maxsim_exact_cpu.py checks the table, tests/test_maxsim_exact_gpu.py runs it.

Exactness: token values k / 8 with |k| <= 4, so a dot product over E <= 768 elements is a multiple of 1/64 with |<q, d>| <= 192, a
score is a sum of at most 64 per-token maxima (or -1000 sentinels): a multiple of 1/64 far below 2^24 / 64, exact in fp32 in any
summation order.  grad_out in {+-1, +-0.5, +-2} makes every gradient a multiple of 1/16 far below 2^24 / 16.  The values
themselves are exact in bf16, fp16 and fp32.  What is left to a kernel is WHICH rows enter the maximum and, in the backward, which
row is the arg-max: exactly what the planted rows pin.

Planted rows: pattern vectors of +-0.5 (`pats[k]`, pairwise distinct).  <pat, pat> = E / 4 is the largest dot product any two
rows of this value set can have, and only an identical row reaches it.  Query token PTOK[k] of every query holds pats[k]; a
document row that holds pats[k] is then the strict unique maximum of that token, wherever it sits.  Edge kinds (Edge.kind):

    row        an unmasked row holds pats[k]: it decides token k's maximum           mutation: the row leaves the max
    pad        the first padded row (row `len`; row 0 of a fully padded document) holds pats[k], no unmasked row does
                                                                                      mutation: the row is admitted
    hole       a masked row inside the document holds pats[k], no unmasked row does  mutation: the hole is admitted
    hole_copy  (backward) a masked row holds pats[k] and a LATER unmasked row too: the later copy takes the gradient
                                                                                      mutation: the hole is admitted
    dup        two unmasked copies of pats[k] far apart: the score is that of one; in the backward the first takes all the
               gradient, the second exactly none         mutation: forward both leave the max; backward the first leaves it
    pre        (ragged) the store row in front of the document's range holds pats[k]  mutation: the range begins one row early
    qtok       a planted query token whose document row exists                        mutation: the token is masked
    qpad       a padded query token / a hole in a query mask that holds pats[0]       mutation: the token is admitted

Every mutation is a change of one mask bit (two for a forward `dup`) of the restatement's inputs: `mutated_masks`.
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import np_oracle as O
from tests import maxsim_inbatch_bwd_reference as R

GO_VALUES = np.array([1.0, -1.0, 0.5, -0.5, 2.0, -2.0])
N_PAT = 6                                       # planted query tokens per query (fewer when Q is smaller)
ENCODINGS = ("len", "i64", "u8", "bool", "f32")  # what ops._mask accepts: 1-D lengths, int64, uint8, bool, float32


class Edge(NamedTuple):
    kind: str
    doc: int          # pair index (maxsim, ragged, bwd) or document index (inbatch); -1 for query-side edges
    rows: tuple       # document rows of the restatement's d that hold the pattern
    k: int            # pattern index
    query: int        # query index
    tok: int          # query token PTOK[k] (qpad: the padded token)


class Case:
    """One exact case.  q [nq, Q, E], d [B, D, E] float64; qm [nq, Q], dm [B, D] int64 (0 / 1).  entry:
    maxsim   pair p scores against query p // ppq
    inbatch  all pairs, q [Bq], d [Bd]; bug = the reference's masking by document i
    ragged   tokens [T, E], begin / end [B]; d / dm are the padded restatement: d[p] = tokens[begin[p] - 1 : begin[p] - 1 + D]
             (zeros past the store), dm[p, 1 : 1 + len] = 1, so row 0 is the store row in front of the range
    bwd      pair per row, go [B]"""

    def __init__(self, **kw):
        self.ppq, self.bug, self.go, self.tokens, self.begin, self.end = 1, False, None, None, None, None
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def row_name(row):
    """The id of a TABLE row (and the name of its case) without building it."""
    entry, tag, dtype, Q, D, E, batch, enc, seed = row
    shape = "store" if entry == "ragged" else "x".join(str(int(b)) for b in batch)
    return f"{entry}-{tag}-{dtype}-Q{Q}-D{D}-E{E}-{shape}-{enc}"


# ------------------------------------------------------------------------------------------------------------- building blocks
def planted_tokens(Q):
    """The query tokens that hold patterns: 0, Q - 1, 31, 32 where Q allows, then the lowest free ones, N_PAT at most."""
    tok = []
    for t in (0, Q - 1, 31, 32):
        if 0 <= t < Q and t not in tok:
            tok.append(t)
    t = 1
    while len(tok) < min(Q, N_PAT):
        if t not in tok:
            tok.append(t)
        t += 1
    return tok


def _patterns(rng, n, E):
    pats = []
    while len(pats) < n:
        p = rng.integers(0, 2, E) - 0.5
        if all((p != o).any() for o in pats):
            pats.append(p)
    return np.array(pats)


def _draw(rng, *shape):
    return rng.integers(-4, 5, shape).astype(np.float64) / 8


def _prefix_lens(D):
    out = []
    for L in (D - 1, 33, 32, 1, 31, D // 2 + 1):
        if 1 <= L < D and L not in out:
            out.append(L)
    return out


def _edge_rows(L):
    """The rows of a document of L valid rows that a kernel gets wrong first: row 0, the last one, 31 and 32 (the block
    boundary), the first row of the last block."""
    pos = []
    for r in (0, L - 1, 31, 32, 32 * ((L - 1) // 32)):
        if 0 <= r < L and r not in pos:
            pos.append(r)
    return pos


def _plan_doc(D, role, rot, holes_ok, bwd, rng):
    """-> (mask [D], [(kind, rows)]) of one padded document.  role: 0 len == D, 1 / 4 prefix lengths, 2 fully padded,
    3 a non-prefix mask (holes); rot rotates the choice of lengths and rows in tables of more than five pairs."""
    lens = _prefix_lens(D)
    mask = np.ones(D, np.int64)
    off = {1: 0, 4: 1, 3: 2}.get(role, 0)
    if role == 3 and holes_ok and D >= 7:
        h, c, r1, r2 = D // 3, D - 2, 1, D - 1
        mask[h] = 0
        free = [r for r in range(D) if r not in (0, h, c, r1, r2)]
        for r in rng.choice(free, size=min(2, len(free)), replace=False):
            mask[r] = 0
        return mask, [("row", (0,)), ("hole_copy", (h, c)) if bwd else ("hole", (h,)), ("dup", (r1, r2))]
    if role == 2:
        mask[:] = 0
        return mask, [("pad", (0,))]
    if role == 0 or not lens:
        pos = _edge_rows(D)
        s = rot % len(pos)
        return mask, [("row", (r,)) for r in pos[s:] + pos[:s]]
    L = lens[(rot + off) % len(lens)]
    mask[L:] = 0
    plan = [("row", (L - 1,)), ("pad", (L,))]
    if role == 1:
        plan += [("row", (r,)) for r in _edge_rows(L) if r != L - 1]
    elif L >= 5:
        plan.append(("dup", (1, L - 2)))
    return mask, plan


def _query_masks(rng, nq, Q, holes_ok, ptok, kinds=(0, 1, 2)):
    """[nq, Q]: query i of kind kinds[i % len(kinds)]: 0 full, 1 a padded tail, 2 holes (a shorter prefix where the encoding has
    none); and the padded tokens that get pats[0] (the first padded one / each hole), as (query, token)."""
    qm = np.ones((nq, Q), np.int64)
    padded = []
    free = [t for t in range(Q) if t not in ptok]
    for i in range(nq):
        kind = kinds[i % len(kinds)]
        if kind == 1 and Q >= 2:
            L = max(1, Q - 2)
            qm[i, L:] = 0
            padded.append((i, L))
        elif kind == 2 and holes_ok and free:
            for t in {free[0], free[-1]}:
                qm[i, t] = 0
                padded.append((i, t))
        elif kind == 2 and Q >= 2:
            L = 33 if Q > 33 else 32 if Q > 32 else max(1, Q // 2)
            qm[i, L:] = 0
            padded.append((i, L))
    return qm, padded


def _plant_queries(q, qm, padded, pats, ptok):
    for k, t in enumerate(ptok):
        q[:, t] = pats[k]
    edges = []
    for i, t in padded:
        if t not in ptok:
            q[i, t] = pats[0]
        edges.append(Edge("qpad", -1, (), 0, i, t))
    return edges


def _plant_doc(d_row, plan, pool, pats, doc, query, ptok):
    edges = []
    for (kind, rows), k in zip(plan, pool):
        for r in rows:
            d_row[r] = pats[k]
        edges.append(Edge(kind, doc, tuple(rows), k, query, ptok[k]))
    return edges


def _qtok_edges(edges):
    seen, out = set(), []
    for e in edges:
        if e.kind == "row" and (e.query, e.k) not in seen:
            seen.add((e.query, e.k))
            out.append(Edge("qtok", e.doc, e.rows, e.k, e.query, e.tok))
    return out


# ------------------------------------------------------------------------------------------------------------- the builders
@functools.lru_cache(maxsize=None)
def build(entry, tag, dtype, Q, D, E, batch, enc, seed):
    """One case from (layout, dtype, Q, D, E, batch shape, mask encoding, seed).  batch: maxsim (n_pairs, ppq); bwd (n_pairs,);
    inbatch (Bq, Bd, bug); ragged (document lengths, candidates per query as tuples of document indices)."""
    rng = np.random.default_rng(seed)
    holes_ok = enc != "len"
    ptok = planted_tokens(Q)
    pats = _patterns(rng, len(ptok), E)
    kw = dict(entry=entry, tag=tag, dtype=dtype, Q=Q, D=D, E=E, enc=enc, seed=seed, ptok=ptok, pats=pats,
              name=row_name((entry, tag, dtype, Q, D, E, batch, enc, seed)))
    if entry == "ragged":
        return _build_ragged(rng, kw, batch, holes_ok)
    if entry == "inbatch":
        Bq, Bd, bug = batch
        nq, B, ppq = Bq, Bd, 1
    else:
        B, ppq = batch if entry == "maxsim" else (batch[0], 1)
        nq, bug = (B + ppq - 1) // ppq, False
    q, d = _draw(rng, nq, Q, E), _draw(rng, B, D, E)
    # (backward: a fully padded document, pair 2 of 5, carries no gradient whatever its query mask: it gets the full one)
    qm, padded = _query_masks(rng, nq, Q, holes_ok, ptok, (0, 1, 0, 2, 1) if entry == "bwd" else (0, 1, 2))
    edges = _plant_queries(q, qm, padded, pats, ptok)
    dm = np.ones((B, D), np.int64)
    for p in range(B):
        # all pairs: query 0 has the full mask and meets every document; bug-compatible: document p's mask acts on query p
        query = (p if bug else 0) if entry == "inbatch" else p // ppq
        pool = [k for k in range(len(ptok)) if qm[query, ptok[k]]]
        dm[p], plan = _plan_doc(D, p % 5, p // 5, holes_ok, entry == "bwd", rng)
        edges += _plant_doc(d[p], plan, pool, pats, p, query, ptok)
    edges += _qtok_edges(edges)
    go = rng.choice(GO_VALUES, B) if entry == "bwd" else None
    return Case(q=q, d=d, qm=qm, dm=dm, go=go, ppq=ppq, bug=bug, edges=edges, **kw)


def _build_ragged(rng, kw, batch, holes_ok):
    lens, cands = batch
    Q, E, ptok, pats = kw["Q"], kw["E"], kw["ptok"], kw["pats"]
    n_pat = len(ptok)
    assert n_pat >= 4, "the ragged cases keep two patterns for the rows around a range"
    k_pre, k_pad = n_pat - 2, n_pat - 1
    # the store: [row in front][document rows][row behind] per document; the last document ends the store (tail clamp)
    rows, begin, end, doc_edges = [], [], [], []
    for j, L in enumerate(lens):
        rows.append(pats[k_pre][None])
        begin.append(sum(len(r) for r in rows))
        body = _draw(rng, L, E)
        plan = [("row", (r,)) for r in _edge_rows(L)]
        doc_edges.append([(kind, rws, k) for (kind, rws), k in zip(plan, range(n_pat - 2))])
        for kind, rws, k in doc_edges[-1]:
            body[rws[0]] = pats[k]
        rows.append(body)
        end.append(begin[-1] + L)
        if j + 1 < len(lens):
            rows.append(pats[k_pad][None])
    assert lens[-1] > 0
    tokens = np.concatenate(rows)
    nq = len(cands)
    ppq = len(cands[0])
    flat = [c for row in cands for c in row]
    B = len(flat)
    assert all(len(r) == ppq for r in cands[:-1]) and 1 <= len(cands[-1]) <= ppq and nq == (B + ppq - 1) // ppq
    D = max(lens) + 2
    q = _draw(rng, nq, Q, E)
    qm, padded = _query_masks(rng, nq, Q, holes_ok, ptok)
    edges = _plant_queries(q, qm, padded, pats, ptok)
    d, dm = np.zeros((B, D, E)), np.zeros((B, D), np.int64)
    for p, j in enumerate(flat):
        src = tokens[begin[j] - 1: begin[j] - 1 + D]
        d[p, : len(src)] = src
        dm[p, 1: 1 + lens[j]] = 1
        query = p // ppq
        valid = lambda k: bool(qm[query, ptok[k]])
        for kind, rws, k in doc_edges[j]:
            if valid(k):
                edges.append(Edge(kind, p, (rws[0] + 1,), k, query, ptok[k]))
        if valid(k_pre):
            edges.append(Edge("pre", p, (0,), k_pre, query, ptok[k_pre]))
        if valid(k_pad) and j + 1 < len(lens):
            edges.append(Edge("pad", p, (1 + lens[j],), k_pad, query, ptok[k_pad]))
    edges += _qtok_edges(edges)
    b, e = np.array(begin, np.int64)[flat], np.array(end, np.int64)[flat]
    kw["D"] = D
    return Case(q=q, d=d, qm=qm, dm=dm, ppq=ppq, edges=edges, tokens=tokens, begin=b, end=e, lens=tuple(lens), cand=tuple(flat), **kw)


# ------------------------------------------------------------------------------------------------------------- expectation
def expect(case, qm=None, dm=None, pairs=None):
    """The float64 expectation, optionally with other masks and for a subset: `pairs` = pair indices (maxsim, ragged, bwd) or
    document indices (inbatch without bug-compatible masking).  maxsim / ragged: scores [len(pairs)]; inbatch: [Bq, len(pairs)];
    bwd: (grad_q [n, Q, E], grad_d [n, D, E])."""
    qm = case.qm if qm is None else qm
    dm = case.dm if dm is None else dm
    if case.entry == "inbatch":
        if pairs is None or case.bug:
            out = O.maxsim_inbatch(case.q, qm, case.d, dm, bug_compatible=case.bug, dtype=np.float64)
            return out if pairs is None else out[:, pairs]
        return O.maxsim_inbatch(case.q, qm, case.d[pairs], dm[pairs], dtype=np.float64)
    pairs = np.arange(case.d.shape[0]) if pairs is None else np.asarray(pairs)
    qi = pairs // case.ppq
    if case.entry != "bwd":
        return O.maxsim_paired(case.q[qi], case.d[pairs], qm[qi], dm[pairs], dtype=np.float64)
    gq = np.zeros((len(pairs),) + case.q.shape[1:])
    gd = np.zeros((len(pairs),) + case.d.shape[1:])
    for n, p in enumerate(pairs):                     # the all-pairs restatement on a 1 x 1 batch, pair by pair
        g = R.gradients(case.q[p:p + 1], qm[p:p + 1], case.d[p:p + 1], dm[p:p + 1], case.go[p:p + 1, None])
        gq[n], gd[n] = g["gq"][0], g["gd"][0]
    return gq, gd


def take(case, out, sel):
    """The part of a full expectation that expect(..., pairs=sel) recomputes."""
    if sel is None:
        return out
    if case.entry == "inbatch":
        return out[:, sel]
    return (out[0][sel], out[1][sel]) if case.entry == "bwd" else out[sel]


def mutated_masks(case, edge):
    """(qm, dm, affected pairs / documents) with the one edge mutated (module docstring)."""
    qm, dm = case.qm.copy(), case.dm.copy()
    if edge.kind in ("qtok", "qpad"):
        qm[edge.query, edge.tok] = 1 if edge.kind == "qpad" else 0
        if case.entry == "inbatch":
            return qm, dm, None
        B = case.d.shape[0]
        return qm, dm, [p for p in range(edge.query * case.ppq, min(B, (edge.query + 1) * case.ppq))]
    if edge.kind == "row":
        dm[edge.doc, edge.rows[0]] = 0
    elif edge.kind in ("pad", "hole", "hole_copy", "pre"):
        dm[edge.doc, edge.rows[0]] = 1
    elif edge.kind == "dup":
        dm[edge.doc, edge.rows[0]] = 0
        if case.entry != "bwd":
            dm[edge.doc, edge.rows[1]] = 0
    else:
        raise ValueError(edge.kind)
    return qm, dm, (None if case.bug else [edge.doc])       # (bug-compatible masking: document i's mask acts on row i)


# ------------------------------------------------------------------------------------------------------------- dispatch
K_CUS = 256                                      # launch_geometry.h: kCUs


def wave_split(n, max_waves):
    """launch_geometry.h wave_split -> (pairs per wavefront, grid)."""
    if n <= 0:
        return 1, 0
    waves = min(max(max_waves, 1), n)
    per = (n + waves - 1) // waves
    return per, (n + per - 1) // per


def stream_width(E):                             # launch_geometry.h stream_width
    return E in (128, 256, 384, 512, 768)


def expected_kernel(case):
    """The kernel the default environment (no MM_MAXSIM_* switch) runs for `case`, as "<kernel>" or "<kernel>:<way in>".
    A restatement, line by line, of
      maxsim.hip      mm_maxsim_fwd (pair_kernel / stream_ok / kp128 / launch_generic order), launch_stream (the NQT == 2 in-kernel
                      mask forms), launch_stream_nsl (Q > 32 -> two tiles), stream_one_pair_per_wave, stream_max_waves (4 per CU),
                      mm_maxsim_inbatch_fwd + launch_stream_inb_cfg, mm_maxsim_ragged_fwd, mm_maxsim_bwd (a.row_masks)
      maxsim_pair.hip maxsim_pair_supported, maxsim_pair_i64_supported (torch allocations are 16-byte aligned), launch_pair
                      (wave_split over 256 * 4 wavefronts)
      kernel_pool128.hip kp128_maxsim_supported
    It serves only to show that the table reaches every branch."""
    f32 = case.dtype == "f32"
    Q, D, E = case.Q, case.D, case.E
    streams = not f32 and Q <= 64 and stream_width(E)            # stream_ok
    waves = K_CUS * 4
    if case.entry == "bwd":
        lds = Q * 4 + 2 * 128 * 4
        return "bwd_rowmasks" if lds + D * ((Q + 31) // 32) * 4 <= 60 * 1024 else "bwd_scan"
    if case.entry == "ragged":
        if streams:
            return "rag_stream2" if Q > 32 else "rag_stream1"
        return "rag_generic:" + ("f32" if f32 else "width")
    if case.entry == "inbatch":
        Bq, Bd = case.q.shape[0], case.d.shape[0]
        if not streams:
            return "inb_generic"
        if Q <= 32 and not case.bug and Bq > 1 and E in (128, 256):
            return "inb_ring" if Bq >= 64 and Bd >= 64 else "inb_tiled"
        return "inb_untiled:" + ("Q>32" if Q > 32 else "bug" if case.bug else "Bq=1" if Bq == 1 else "width")
    B, ppq = case.d.shape[0], case.ppq
    i64 = case.enc == "i64"
    split = wave_split(B, waves)[0] > 1
    pair = ppq == 1 and not f32 and Q <= 32 and stream_width(E)  # maxsim_pair_supported
    if pair and i64 and 2 <= D <= 256 and Q >= 2 and D % 2 == 0 and Q % 2 == 0:
        return "pair_i64" + (":split" if split else "")
    if streams and not pair and Q > 32 and D <= 256 and i64 and not split:
        if B * 2 <= waves and D > 32:
            return "stream2_i64_wpp2"
        return "stream2_i64_wpp1:" + ("D<=32" if D <= 32 else "pairs")
    if pair:
        way = ":split" if split else ":D>256" if i64 and D > 256 else ":odd" if i64 else ""
        return "pair_packed" + way
    if streams:
        return ("stream2_packed" if Q > 32 else "stream1") + (":split" if split else "")
    if f32 and Q <= 32 and E % 64 == 0 and E // 64 in (1, 2, 3, 4, 6, 8, 12):   # kp128_maxsim_supported
        return "f32_split"
    return "generic:" + ("f32-Q>32" if f32 and Q > 32 else "f32-width" if f32 else "16bit-Q>64" if Q > 64 else "16bit-width")


B16 = ("bf16", "fp16")
# every branch the table must reach -> the dtypes it must reach it with
REQUIRED = {
    "pair_packed": B16, "pair_packed:odd": B16, "pair_packed:D>256": B16, "pair_packed:split": B16,
    "pair_i64": B16, "pair_i64:split": B16,
    "stream1": B16, "stream1:split": B16, "stream2_packed": B16,
    "stream2_i64_wpp2": B16, "stream2_i64_wpp1:D<=32": B16, "stream2_i64_wpp1:pairs": B16,
    "f32_split": ("f32",),
    "generic:f32-Q>32": ("f32",), "generic:f32-width": ("f32",), "generic:16bit-width": B16, "generic:16bit-Q>64": B16,
    "inb_ring": B16, "inb_tiled": B16, "inb_untiled:Q>32": B16, "inb_untiled:width": B16, "inb_untiled:Bq=1": B16,
    "inb_untiled:bug": B16, "inb_generic": ("f32",),
    "rag_stream1": B16, "rag_stream2": B16, "rag_generic:f32": ("f32",), "rag_generic:width": B16,
    "bwd_rowmasks": ("bf16", "fp16", "f32"), "bwd_scan": ("f32",),
}

# MM_MAXSIM_* switch (EnvCfg in mm_internal.h) -> the kernels (expected_kernel without the way in) whose cases it reroutes
SWITCHES = {
    "MM_MAXSIM_GENERIC=1": None,                 # every forward case
    "MM_MAXSIM_NBUF=3": ("pair_packed", "pair_i64", "stream1"),
    "MM_MAXSIM_NBUF=4": ("pair_packed", "pair_i64", "stream1"),
    "MM_MAXSIM_NT=0": ("stream1",),
    "MM_MAXSIM_WPC=1": ("pair_packed", "pair_i64", "stream1", "stream2_packed", "stream2_i64_wpp2", "stream2_i64_wpp1",
                        "rag_stream1", "rag_stream2"),
    "MM_MAXSIM_NO_WPP2=1": ("stream2_i64_wpp2",),
    "MM_MAXSIM_NO_INLINE_MASKS=1": ("stream2_i64_wpp2", "stream2_i64_wpp1"),
    "MM_MAXSIM_INB_UNTILED=1": ("inb_ring", "inb_tiled"),
    "MM_MAXSIM_INB_NOWG=1": ("inb_ring",),
}


# ------------------------------------------------------------------------------------------------------------- the table
def _table():
    """(entry, tag, dtype, Q, D, E, batch, enc) rows; the seed is the row's position."""
    t = []
    add = lambda *row: t.append(row)
    packed = ("len", "u8", "f32", "bool", "u8")
    for dt in B16:
        # ops.maxsim, pair-per-row layout (ppq = 1, Q <= 32)
        for n, (Q, D, E) in enumerate([(32, 33, 128), (7, 31, 256), (1, 1, 384), (20, 64, 512), (32, 65, 768)]):
            add("maxsim", "pair", dt, Q, D, E, (5, 1), packed[n])
        for Q, D, E in [(32, 34, 128), (2, 2, 128), (8, 64, 384), (30, 256, 768)]:
            add("maxsim", "pair", dt, Q, D, E, (4, 1), "i64")
        add("maxsim", "pair", dt, 32, 258, 128, (5, 1), "i64")       # D > 256: int64 masks are packed
        add("maxsim", "pair", dt, 32, 33, 128, (5, 1), "i64")        # odd D: int64 masks are packed
        add("maxsim", "pair", dt, 4, 34, 128, (1025, 1), "i64")      # 1,024 wavefronts of two pairs and one of a single pair
        add("maxsim", "pair", dt, 4, 34, 128, (1025, 1), "len")
        # shared-query layout (ppq > 1): the streaming kernels; 11 pairs in groups of 3 leave a short last group
        for n, E in enumerate((128, 256, 384, 512, 768)):
            add("maxsim", "shared", dt, (32, 7, 20, 4, 31)[n], (33, 65)[n % 2], E, (11, 3), ("u8", "len", "i64", "f32", "bool")[n])
        add("maxsim", "shared", dt, 3, 33, 128, (1025, 5), "len")
        for n, (Q, D, E) in enumerate([(33, 47, 128), (64, 40, 256), (38, 33, 768)]):
            add("maxsim", "two-tile", dt, Q, D, E, (5, 1), ("len", "u8", "f32")[n])
            add("maxsim", "two-tile", dt, Q, D, E, (7, 3), ("bool", "f32", "len")[n])
        add("maxsim", "two-tile", dt, 38, 34, 128, (4, 1), "i64")
        add("maxsim", "two-tile", dt, 38, 32, 128, (4, 1), "i64")
        add("maxsim", "two-tile", dt, 38, 34, 128, (600, 1), "i64")
        add("maxsim", "generic", dt, 20, 33, 24, (5, 1), "i64")
        add("maxsim", "generic", dt, 20, 33, 640, (5, 1), "u8")
        add("maxsim", "generic", dt, 65, 33, 128, (5, 1), "len")
        # ops.maxsim_inbatch
        for E in (128, 256):
            add("inbatch", "ring", dt, 5, 33, E, (67, 70, False), "i64" if E == 128 else "len")
            add("inbatch", "tiled", dt, 5, 33, E, (3, 5, False), "u8" if E == 128 else "f32")
        add("inbatch", "untiled", dt, 33, 33, 128, (3, 5, False), "i64")
        add("inbatch", "untiled", dt, 5, 33, 384, (3, 5, False), "bool")
        add("inbatch", "untiled", dt, 5, 33, 128, (1, 5, False), "len")
        add("inbatch", "untiled", dt, 5, 33, 128, (5, 5, True), "i64")
        # ops.maxsim_ragged: ranges that begin and end inside a 32-row block, an empty one, the store's last document, repeats
        lens = (33, 0, 1, 32, 47, 31, 64, 65, 5)
        cands = ((0, 1, 7, 8, 3, 3), (4, 5, 6, 2, 8, 1), (4, 5, 6, 7))
        add("ragged", "one-tile", dt, 20, 0, 128, (lens, cands), "len")
        add("ragged", "one-tile", dt, 7, 0, 768, (lens, cands), "u8")
        add("ragged", "two-tile", dt, 38, 0, 256, (lens, cands), "i64")
        add("ragged", "generic", dt, 7, 0, 40, (lens, cands), "f32")
    for n, (Q, D, E) in enumerate([(32, 33, 64), (7, 31, 128), (20, 65, 384), (5, 33, 768)]):
        add("maxsim", "fp32", "f32", Q, D, E, (5, 1) if n % 2 == 0 else (11, 3), ("i64", "len", "u8", "f32")[n])
    add("maxsim", "generic", "f32", 40, 33, 128, (5, 1), "bool")
    add("maxsim", "generic", "f32", 20, 33, 24, (7, 3), "i64")
    add("inbatch", "generic", "f32", 5, 33, 128, (3, 5, False), "i64")
    add("inbatch", "generic", "f32", 5, 33, 128, (4, 4, True), "f32")
    add("ragged", "generic", "f32", 20, 0, 128, (lens, cands), "bool")
    # ops.maxsim_bwd
    bwd_enc = ("i64", "len", "u8", "f32", "bool", "i64")
    for dt in ("bf16", "fp16", "f32"):
        for n, (Q, D, E) in enumerate([(13, 47, 64), (40, 70, 24), (32, 180, 128), (8, 33, 768), (70, 95, 16), (1, 1, 8)]):
            add("bwd", "pair", dt, Q, D, E, (5,), bwd_enc[n])
    add("bwd", "pair", "f32", 320, 1540, 8, (5,), "i64")            # D x ceil(Q / 32) words exceed the LDS row masks
    return [row + (seed,) for seed, row in enumerate(t)]


TABLE = _table()


def cases(entry=None):
    return [build(*row) for row in TABLE if entry is None or row[0] in entry]


def case_by_name(name):
    return {c.name: c for c in cases()}[name]
