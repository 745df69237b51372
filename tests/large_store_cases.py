"""The two 4 GiB buffers of tests/test_large_store_gpu.py, the views the retrieval operators take of them, and the row
windows that straddle the three lines where 32-bit addressing breaks:

    b31  the first row whose BYTE offset reaches 2^31   (signed 32-bit byte arithmetic goes negative)
    b32  the first row whose byte offset reaches 2^32   (unsigned 32-bit byte arithmetic wraps)
    e31  the first row whose ELEMENT index reaches 2^31 (signed 32-bit element arithmetic goes negative)

Everything here is host arithmetic (numpy): tests/test_large_store_cases_cpu.py proves, from these tables alone, that every
window lies where its name says and that every operator of the GPU module touches a row beyond the lines of its store.  The
fill functions at the end are the only device code; they import torch when called.

Data.  X16 holds multiples of 1/4 in [-1/2, 1/2], C8 the e4m3fn bytes of the same values, S8 powers of two in 2^-3 .. 2^3;
queries, centroids and codebooks use the same value set.  In the unit of the smallest product (1/16 of the smallest scale)
every dot product, scaled or not, is an integer below EXACT_LIMIT = 2^24: exact in fp32 in any summation order (the
project's `ternary` / `quarter` / exact stores work the same way)."""
import collections
import fractions
import math

import numpy as np

E = 128                                    # the width both buffers are allocated with
N16 = 2 ** 24 + 6002                       # X16 [N16, 128] float16: 4.00 GiB
N8 = 2 ** 25 + 6004                        # C8 [N8, 128] uint8: 4.00 GiB; S8 [N8] float32
WIDE = 768                                 # the second view of both buffers
AH_BYTES = WIDE // 4                       # an ah_scan code row for E = 768

VALUE_NUM = (-2, -1, 0, 1, 2)              # X16 / C8 / query / centroid / codebook entries, over
VALUE_DEN = 4
SCALE_EXP = (-3, 3)                        # S8 = 2^k, k in this closed range
EXACT_LIMIT = 2 ** 24

B31, B32, E31 = "b31", "b32", "e31"
LINE_VALUE = {B31: 2 ** 31, B32: 2 ** 32, E31: 2 ** 31}

SEED_X16, SEED_C8, SEED_S8 = 1601, 801, 802
FILL_CHUNK = 1 << 20                       # rows generated per step
CHUNK = 1 << 20                            # rows per slice of the big == chunks comparisons
MIN_FREE_BYTES = 24e9                      # the module skips below this much free device memory

View = collections.namedtuple("View", "name buffer rows row_bytes row_elems")
#   row_elems = 0: the operator indexes this view by bytes (or by 4-byte words of one row) only, there is no element line

VIEWS = {v.name: v for v in (
    View("x16_e128", "X16", N16, 2 * E, E),
    View("x16_e768", "X16", N16 * E // WIDE, 2 * WIDE, WIDE),
    View("c8_e128", "C8", N8, E, E),
    View("c8_e768", "C8", N8 * E // WIDE, WIDE, WIDE),
    View("c8_ah768", "C8", N8 * E // AH_BYTES, AH_BYTES, 0),        # [n, E / 4] codes of ah_scan, E = 768
    View("nbr_m64", "NBR", N16, 4 * 64, 0),                         # graph_search's neighbours [N16, 64] int32
    View("q8_e128", "OUT", N16, E, E),                              # fp8 codes written for X16 (fp8_quantize_rows, store_append)
)}

Window = collections.namedtuple("Window", "name lo hi lines first")
#   lines: the lines this window straddles (() for the start and the tail); first: the first row at or past them

BELOW, ABOVE, TAIL = 4000, 400, 500        # rows of a straddling window below / from its line on; rows of the tail window


def row_unit(view, line):
    """what one row of `view` advances towards `line`: bytes, or elements"""
    return view.row_elems if line == E31 else view.row_bytes


def line_rows(view):
    """{line: exact row number (a Fraction) at which the line falls} for the lines inside the view"""
    out = {}
    for line, value in LINE_VALUE.items():
        unit = row_unit(view, line)
        if unit and view.rows * unit > value:
            out[line] = fractions.Fraction(value, unit)
    return out


def windows(view):
    """The view's windows in ascending row order: start, one per distinct line position, tail.  Lines that fall on one row
    number share a window."""
    at = collections.OrderedDict()
    for line, pos in sorted(line_rows(view).items(), key=lambda kv: (kv[1], kv[0])):
        at.setdefault(math.ceil(pos), []).append(line)
    out = [Window("start", 0, BELOW + ABOVE, (), None)]
    for first, lines in at.items():
        out.append(Window("+".join(lines), first - BELOW, first + ABOVE, tuple(lines), first))
    out.append(Window("tail", view.rows - TAIL, view.rows, (), None))
    return out


def window(view, line):
    """the window of `view` that straddles `line`"""
    return next(w for w in windows(view) if line in w.lines)


def compact_rows(ws):
    """[sum of the window lengths] int64: the big-store row of every row of the compact store built from windows ws"""
    return np.concatenate([np.arange(w.lo, w.hi, dtype=np.int64) for w in ws])


def to_compact(rows, ws):
    """big-store rows -> rows of the compact store (-1 stays -1; a row outside every window is an error)"""
    rows = np.asarray(rows, np.int64)
    big = compact_rows(ws)
    pos = np.searchsorted(big, np.maximum(rows, 0))
    pos = np.minimum(pos, big.size - 1)
    assert ((big[pos] == rows) | (rows < 0)).all(), "a row outside the windows"
    return np.where(rows < 0, rows, pos)


def to_big(rows, ws):
    rows = np.asarray(rows, np.int64)
    return np.where(rows < 0, rows, compact_rows(ws)[np.maximum(rows, 0)])


# ---------------------------------------------------------------------------------------------- exactness
def exact_bound(width, scaled):
    """The largest |dot product| over `width` elements, in the unit of the smallest product: values and queries are
    multiples of 1/VALUE_DEN up to max|VALUE_NUM|, and a row scale spans 2^(SCALE_EXP[1] - SCALE_EXP[0]) units."""
    top = max(abs(v) for v in VALUE_NUM)
    return width * top * top * (2 ** (SCALE_EXP[1] - SCALE_EXP[0]) if scaled else 1)


# ---------------------------------------------------------------------------------------------- IVF-style list layouts
SMALL_LENS = [0, 1, 15, 16, 17, 31, 32, 33]        # tests/test_ivf_gpu.py's short lists: empty, one row, around 16 and 32
STRADDLE = (300, 200)                               # rows of the straddling list below / from the line on
LAST_LIST = 333                                     # the list that ends a window without a line (tail: the store's last row)

ListLayout = collections.namedtuple("ListLayout", "windows lens begin_compact begin_big big_of_compact roles")
#   lens / begin_compact: the lists of the compact store; begin_big: the same lists in place in the big store, with one
#   filler list (never probed) per gap between windows; big_of_compact[l] = list l's number there;
#   roles[window name] = {"below" | "straddle" | "above" | "last": compact list number}


def list_layout(view):
    ws = windows(view)
    lens, roles, big_begin, big_of = [], {}, [0], []
    at = 0
    for w in ws:
        if w.lo > at:                                                      # filler
            big_begin.append(w.lo)
        n = w.hi - w.lo
        if w.lines:
            p = w.first - w.lo
            below = p - sum(SMALL_LENS) - STRADDLE[0]
            mine = SMALL_LENS + [below, 0, sum(STRADDLE), n - p - STRADDLE[1]]
            base = len(lens) + len(SMALL_LENS)
            roles[w.name] = {"below": base, "straddle": base + 2, "above": base + 3}
        else:
            mine = SMALL_LENS + [n - sum(SMALL_LENS) - LAST_LIST, 0, LAST_LIST]
            roles[w.name] = {"last": len(lens) + len(SMALL_LENS) + 2}
        assert sum(mine) == n and min(mine) >= 0
        for ln in mine:
            big_of.append(len(big_begin) - 1)
            big_begin.append(big_begin[-1] + ln)
            lens.append(ln)
        at = w.hi
    assert big_begin[-1] == view.rows
    begin_compact = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return ListLayout(ws, lens, begin_compact, np.asarray(big_begin, np.int64), np.asarray(big_of, np.int32), roles)


IVF_NPROBE = 6
IVF_NQ = (1, 37)
IVF_K = (1, 100)


def probes_for(layout, nq, nprobe=IVF_NPROBE):
    """[nq, nprobe] int32 compact list numbers: query i probes lists i nprobe .. i nprobe + nprobe - 1 (mod the list count), so
    37 queries probe every list several times.  Row 0 probes, around a -1 hole, the list that straddles the LAST line, the
    lists on either side of it, the store's last list and a 33-row list; row 1 (when there is one) probes a 1-row and a
    15-row list only: a union of 16 rows, shorter than k = 100."""
    nlist = len(layout.lens)
    p = ((np.arange(nq)[:, None] * nprobe + np.arange(nprobe)[None, :]) % nlist).astype(np.int32)
    last_line = [w for w in layout.windows if w.lines][-1]
    r = layout.roles[last_line.name]
    p[0] = -1
    p[0, :6] = [r["straddle"], -1, layout.roles["tail"]["last"], SMALL_LENS.index(33), r["above"], r["below"]]
    if nq > 1:
        p[1] = -1
        p[1, 0], p[1, 2] = SMALL_LENS.index(1), SMALL_LENS.index(15)
    return p


def probes_to_big(layout, probes):
    return np.where(probes < 0, probes, layout.big_of_compact[np.maximum(probes, 0)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- MaxSim documents
def maxsim_docs(view):
    """(begin, end) int64, big-store rows: documents of 1 .. 70 rows below, across and above every line of the view, at the
    store's first and last rows, and empty ranges (one of them [n, n))."""
    b, e = [], []

    def doc(lo, n):
        b.append(lo)
        e.append(lo + n)

    n = view.rows
    for w in windows(view):
        if w.name == "start":
            doc(0, 1), doc(0, 70), doc(1, 32), doc(3, 0)
        elif w.name == "tail":
            doc(n - 70, 70), doc(n - 1, 1), doc(n - 34, 33), doc(n, 0)
        else:
            r = w.first
            doc(r - 200, 70), doc(r - 130, 1), doc(r - 1, 1)                 # below
            doc(r - 35, 70), doc(r - 1, 2), doc(r - 64, 65), doc(r - 16, 33)  # across
            doc(r, 1), doc(r + 40, 33), doc(r + 100, 64), doc(r + 200, 17)    # above
            doc(r, 0), doc(r - 7, 0)                                          # empty
    return np.asarray(b, np.int64), np.asarray(e, np.int64)


MAXSIM_Q = 8
MAXSIM_PAIRS_PER_QUERY = 5


# ---------------------------------------------------------------------------------------------- the other shapes
KMEANS_NLIST = 37                  # kmeans_assign, ah_encode centres
SEGMENT_NLIST = 130                # kmeans_segment_sum
GATHER_R = 12
GRAPH = dict(M=64, ef=32, width=4, k=32, n_entry=8, nq=9, iters_lds=16, iters_ws=512)
APPEND_ROWS = (8, 40)              # store_append batch [n_docs, D, 128]
FULL_SCAN = {"dot_topk": dict(view="x16_e768", nq=8, k=1000), "dot_topk_fp8": dict(view="c8_e768", nq=8, k=2000)}
SEARCH = dict(nq=5, Q=8, k=16, top_n=10, row_shard=1 << 20)
DOT_SAMPLE = 16384                 # csrc/dot_topk.hip kDotSample (tests/dot_topk_reference.py SAMPLE)


def segment_list_begin(n=N16, nlist=SEGMENT_NLIST):
    """130 lists over all n rows, every fifth one empty, the others of unequal lengths"""
    w = np.array([0 if l % 5 == 4 else 1 + (l * 7) % 11 for l in range(nlist)], np.int64)
    cut = np.cumsum(w) * n // w.sum()
    cut[-1] = n
    return np.concatenate([[0], cut]).astype(np.int64)


def sample_m(k, n):
    """the expected number of sample rows above the threshold of a one-call flat search"""
    return 2.5 * k * DOT_SAMPLE / n


# Every (operator, view it addresses, lines its test crosses there, how).  `whole` = one call reads or writes every row of the
# view; otherwise the named windows.  colbert_candidates addresses no store: its rows are VALUES up to T = 2^31 - 1.
Case = collections.namedtuple("Case", "op view lines whole")
CASES = [
    Case("ivf_scan", "x16_e128", (B31, B32, E31), False), Case("ivf_scan", "x16_e768", (B31, B32, E31), False),
    Case("ivf_scan_fp8", "c8_e128", (B31, B32, E31), False), Case("ivf_scan_fp8", "c8_e768", (B31, B32, E31), False),
    Case("ah_scan", "c8_ah768", (B31, B32), False),
    Case("gather_dot", "x16_e128", (B31, B32, E31), False), Case("gather_dot", "x16_e768", (B31, B32, E31), False),
    Case("graph_search", "x16_e128", (B31, B32, E31), False), Case("graph_search", "nbr_m64", (B31, B32), False),
    Case("maxsim_ragged", "x16_e128", (B31, B32, E31), False), Case("maxsim_ragged", "x16_e768", (B31, B32, E31), False),
    Case("maxsim_ragged_fp8", "c8_e128", (B31, B32, E31), False), Case("maxsim_ragged_fp8", "c8_e768", (B31, B32, E31), False),
    Case("kmeans_segment_sum", "x16_e128", (B31, B32, E31), True),
    Case("kmeans_assign", "x16_e128", (B31, B32, E31), True), Case("kmeans_assign", "x16_e768", (B31, B32, E31), True),
    Case("fp8_quantize_rows", "x16_e128", (B31, B32, E31), True), Case("fp8_quantize_rows", "q8_e128", (B31, E31), True),
    Case("ah_encode", "x16_e768", (B31, B32, E31), True),
    Case("store_append", "x16_e128", (B31, B32, E31), False), Case("store_append", "q8_e128", (B31, E31), False),
    Case("dot_topk", "x16_e768", (B31, B32, E31), True), Case("dot_topk_fp8", "c8_e768", (B31, B32, E31), True),
    Case("colbert_candidates", None, (), False),
]
# (the sharded TokenStore search hands dot_topk / dot_topk_fp8 slices of 2^20 rows, each addressed from 0: what crosses the
# lines there is Python's shard offset, and the candidate and MaxSim stages, which take the whole store)
OPERATORS = ("dot_topk", "dot_topk_fp8", "ivf_scan", "ivf_scan_fp8", "ah_scan", "ah_encode", "gather_dot", "graph_search",
             "maxsim_ragged", "maxsim_ragged_fp8", "kmeans_assign", "kmeans_segment_sum", "fp8_quantize_rows", "store_append",
             "colbert_candidates")

# the first row count include/mm_native.h has the entry point refuse (None: it documents none — the kernel takes int64 rows
# and never counts them: gather_dot and the ragged MaxSims address row * row bytes in 64 bits, store_append bounds the BATCH
# (n_docs * D < 2^31) and takes an int64 capacity, colbert_candidates bounds n_docs, not T).  ah_encode and fp8_quantize_rows
# launch one workgroup per 16 rows: their limits were refused on the host but not documented before this table was written.
ROW_LIMIT = {"dot_topk": 2 ** 31, "dot_topk_fp8": 2 ** 31, "ivf_scan": 2 ** 31, "ivf_scan_fp8": 2 ** 31, "ah_scan": 2 ** 31,
             "graph_search": 2 ** 31, "kmeans_assign": 2 ** 31, "kmeans_segment_sum": 2 ** 31, "ah_encode": 2 ** 35,
             "fp8_quantize_rows": 2 ** 35 - 15, "gather_dot": None, "maxsim_ragged": None, "maxsim_ragged_fp8": None,
             "store_append": None, "colbert_candidates": None}


def append_fills():
    """store_append: (line, first row of the appended batch): the batch starts 100 rows below the row where rows_out
    [N16, 128] float16 reaches 2^31 bytes (2^23) and 2^32 bytes (2^24; codes_out reaches 2^31 bytes there)."""
    v = VIEWS["x16_e128"]
    return [(line, window(v, line).first - 100) for line in (B31, B32)]


def colbert_documents(T=2 ** 31 - 1):
    """(begin, end) int64 in document order for colbert_candidates at T = 2^31 - 1: runs of documents of 1 .. 9 rows (every
    seventh one empty, a gap after every fifth) at row 0, either side of 2^24 and 2^30, and up to the last row T - 1."""
    b, e = [], []
    for anchor, count in ((0, 60), (2 ** 24 - 150, 80), (2 ** 30 - 150, 80), (T - 2 ** 8, None)):
        at, i = anchor, 0
        while (count is None and at < T) or (count is not None and i < count):
            ln = 0 if i % 7 == 6 else 1 + (i * 5) % 9
            ln = min(ln, T - at)
            b.append(at)
            e.append(at + ln)
            at += ln + (3 if i % 5 == 4 and count is not None else 0)
            i += 1
    order = np.random.default_rng(31).permutation(len(b))                  # document order is not row order
    return np.asarray(b, np.int64)[order], np.asarray(e, np.int64)[order]


def colbert_hits(begin, end, T=2 ** 31 - 1, nq=4, H=96):
    """hit rows [nq, H]: first and last rows of ranges, rows in gaps, T - 1, T, -1, rows far from every document"""
    rng = np.random.default_rng(32)
    live = np.nonzero(end > begin)[0]
    hits = np.full((nq, H), -1, np.int64)
    for i in range(nq):
        d = rng.choice(live, H // 2, replace=False)
        row = np.concatenate([begin[d[: H // 4]], end[d[H // 4:]] - 1, end[d[: H // 8]],        # (end = the next row: a
                              [T - 1, T, -1, 2 ** 24, 2 ** 30, 2 ** 31 - 2 ** 8, 12345678, 0]])  # neighbour's first, or a gap)
        hits[i, : row.size] = row
        hits[i] = hits[i][rng.permutation(H)]
    hits[nq - 1, ::2] = -1
    return hits


# ---------------------------------------------------------------------------------------------- device fills
def _values(torch, shape, g, dev):
    return torch.randint(VALUE_NUM[0], VALUE_NUM[-1] + 1, shape, generator=g, device=dev, dtype=torch.int8)


def fill_x16(dev):
    """X16 [N16, 128] float16 on `dev`: seeded multiples of 1/4 in [-1/2, 1/2], generated there chunk by chunk"""
    import torch
    g = torch.Generator(device=dev).manual_seed(SEED_X16)
    x = torch.empty(N16, E, dtype=torch.float16, device=dev)
    for lo in range(0, N16, FILL_CHUNK):
        hi = min(N16, lo + FILL_CHUNK)
        x[lo:hi] = _values(torch, (hi - lo, E), g, dev).to(torch.float16) / VALUE_DEN
    return x


def fill_c8(dev):
    """(C8 [N8, 128] uint8 = the e4m3fn bytes of such values, by torch's cast; S8 [N8] float32 = 2^k, k in SCALE_EXP)"""
    import torch
    g = torch.Generator(device=dev).manual_seed(SEED_C8)
    c = torch.empty(N8, E, dtype=torch.uint8, device=dev)
    for lo in range(0, N8, FILL_CHUNK):
        hi = min(N8, lo + FILL_CHUNK)
        c[lo:hi] = (_values(torch, (hi - lo, E), g, dev).to(torch.float32) / VALUE_DEN).to(torch.float8_e4m3fn).view(torch.uint8)
    g = torch.Generator(device=dev).manual_seed(SEED_S8)
    table = torch.tensor([2.0 ** k for k in range(SCALE_EXP[0], SCALE_EXP[1] + 1)], dtype=torch.float32, device=dev)
    s = table[torch.randint(0, table.numel(), (N8,), generator=g, device=dev)]      # (a table: no pow() on the device)
    return c, s


def small_values(shape, seed):
    """float32 numpy values of the same set (queries, centroids, codebooks)"""
    return (np.random.default_rng(seed).integers(VALUE_NUM[0], VALUE_NUM[-1] + 1, shape) / VALUE_DEN).astype(np.float32)
