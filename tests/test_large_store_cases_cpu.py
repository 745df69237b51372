"""No GPU: the case tables of tests/large_store_cases.py really cross the lines they are named for, every shape stays
inside the limits include/mm_native.h documents, the workspaces stay small, the value set is exact, and the entry points
refuse the first row count past their limit."""
import fractions
import os

import numpy as np
import pytest

from tests import large_store_cases as C


@pytest.fixture(scope="module")
def L():
    from matchmaker_amd import _lib, build
    build.build()
    return _lib.lib()


def _offset(view, row, line):
    """byte offset (element index for e31) of the first byte (element) of `row`"""
    return row * C.row_unit(view, line)


def test_the_buffers_divide_into_their_views():
    for n in (C.N16, C.N8):
        assert n % 6 == 0 and n % 32 != 0 and (n // 6) % 32 != 0
    assert C.N16 * C.E * 2 >= 2 ** 32 and C.N8 * C.E >= 2 ** 32                    # 4.00 GiB each
    assert C.N16 * C.E * 2 < 2 ** 32 + 2 ** 21 and C.N8 * C.E < 2 ** 32 + 2 ** 21
    for v in C.VIEWS.values():
        base = {"X16": C.N16 * C.E * 2, "C8": C.N8 * C.E, "NBR": C.N16 * 256, "OUT": C.N16 * C.E}[v.buffer]
        assert v.rows * v.row_bytes == base, v.name
        assert v.rows % 32 != 0, v.name                                             # a ragged last 32-row block
    assert C.VIEWS["c8_ah768"].row_bytes * 4 == C.WIDE


def test_the_lines_fall_at_the_rows_the_table_names():
    F = fractions.Fraction
    want = {"x16_e128": {C.B31: 2 ** 23, C.B32: 2 ** 24, C.E31: 2 ** 24},
            "x16_e768": {C.B31: F(2 ** 31, 1536), C.B32: F(2 ** 32, 1536), C.E31: F(2 ** 31, 768)},
            "c8_e128": {C.B31: 2 ** 24, C.B32: 2 ** 25, C.E31: 2 ** 24},
            "c8_e768": {C.B31: F(2 ** 31, 768), C.B32: F(2 ** 32, 768), C.E31: F(2 ** 31, 768)},
            "c8_ah768": {C.B31: F(2 ** 31, 192), C.B32: F(2 ** 32, 192)},
            "nbr_m64": {C.B31: 2 ** 23, C.B32: 2 ** 24},
            "q8_e128": {C.B31: 2 ** 24, C.E31: 2 ** 24}}
    assert {name: C.line_rows(v) for name, v in C.VIEWS.items()} == want
    assert int(want["x16_e768"][C.B31]) == 1398101 and int(want["x16_e768"][C.B32]) == 2796202      # a row straddles each
    assert int(want["c8_e768"][C.B32]) == 5592405


@pytest.mark.parametrize("name", sorted(C.VIEWS))
def test_windows_straddle_their_lines(name):
    v = C.VIEWS[name]
    ws = C.windows(v)
    assert ws[0].name == "start" and ws[0].lo == 0 and ws[-1].name == "tail" and ws[-1].hi == v.rows
    assert (ws[-1].hi - ws[-1].lo) % 32 != 0 and v.rows % 32 != 0
    for a, b in zip(ws, ws[1:]):
        assert a.hi < b.lo                                                          # disjoint, ascending, a gap between
    for w in ws:
        assert 0 <= w.lo < w.hi <= v.rows and 400 <= w.hi - w.lo <= 5000
    seen = set()
    for w in ws[1:-1]:
        assert w.lines
        for line in w.lines:
            seen.add(line)
            value = C.LINE_VALUE[line]
            assert _offset(v, w.lo, line) < value <= _offset(v, w.hi - 1, line), (name, w)
            assert _offset(v, w.first - 1, line) < value <= _offset(v, w.first, line)       # `first` = the first row past it
            assert C.window(v, line) == w
    assert seen == set(C.line_rows(v))
    big = C.compact_rows(ws)
    assert (np.diff(big) > 0).all()
    assert (C.to_compact(big, ws) == np.arange(big.size)).all() and (C.to_big(np.arange(big.size), ws) == big).all()
    assert C.to_compact([-1, ws[-1].hi - 1], ws).tolist() == [-1, big.size - 1]


@pytest.mark.parametrize("name", ["x16_e128", "x16_e768", "c8_e128", "c8_e768", "c8_ah768"])
def test_list_layouts_put_a_list_below_across_and_above_every_line(name):
    v = C.VIEWS[name]
    lay = C.list_layout(v)
    lb, lc = lay.begin_big, lay.begin_compact
    assert lb[0] == 0 and lb[-1] == v.rows and (np.diff(lb) >= 0).all()
    assert len(lay.lens) == len(lay.big_of_compact) == len(lc) - 1
    big_rows = C.compact_rows(lay.windows)
    for l, ln in enumerate(lay.lens):                                               # the same rows, in place
        bl = int(lay.big_of_compact[l])
        assert lb[bl + 1] - lb[bl] == ln == lc[l + 1] - lc[l]
        if ln:
            assert big_rows[lc[l]] == lb[bl] and big_rows[lc[l + 1] - 1] == lb[bl + 1] - 1
    fillers = set(range(len(lb) - 1)) - set(lay.big_of_compact.tolist())
    assert len(fillers) == len(lay.windows) - 1 and all(lb[f + 1] - lb[f] > 0 for f in fillers)
    for want in (0, 1, 15, 16, 17, 31, 32, 33):
        assert want in lay.lens
    assert max(lay.lens) >= 3000
    for w in lay.windows:
        r = lay.roles[w.name]
        if not w.lines:
            last = int(lay.big_of_compact[r["last"]])
            assert lb[last + 1] == w.hi and (lb[last + 1] - lb[last]) % 32 != 0
            continue
        lo = {k: int(lb[lay.big_of_compact[i]]) for k, i in r.items()}
        hi = {k: int(lb[lay.big_of_compact[i] + 1]) for k, i in r.items()}
        for line in w.lines:
            value = C.LINE_VALUE[line]
            assert _offset(v, hi["below"] - 1, line) < value and hi["below"] - lo["below"] >= 3000
            assert _offset(v, lo["straddle"], line) < value <= _offset(v, hi["straddle"] - 1, line)
            assert _offset(v, lo["above"], line) >= value and hi["above"] > lo["above"]
    for nq in C.IVF_NQ:
        p = C.probes_for(lay, nq)
        assert p.shape == (nq, C.IVF_NPROBE) and p.max() < len(lay.lens) and (p[0] == -1).sum() == 1
        for row in p:
            live = row[row >= 0]
            assert len(set(live.tolist())) == live.size                             # no list twice in a row
        pb = C.probes_to_big(lay, p)
        assert not set(pb[pb >= 0].tolist()) & fillers
        if nq > 1:
            assert sum(lay.lens[l] for l in p[1] if l >= 0) == 16 < max(C.IVF_K)
            assert set(p[p >= 0].tolist()) == set(range(len(lay.lens)))             # every list is probed by someone


def test_every_operator_crosses_the_lines_of_its_store():
    assert {c.op for c in C.CASES} == set(C.OPERATORS) and len(C.OPERATORS) == 15
    for c in C.CASES:
        if c.view is None:
            continue
        v = C.VIEWS[c.view]
        assert set(c.lines) == set(C.line_rows(v)), c                               # ... every line the view has
        assert C.B31 in c.lines, c
        for line in c.lines:
            value = C.LINE_VALUE[line]
            if c.whole:
                last = v.rows - 1
            elif c.op == "store_append":
                last = max(f for _, f in C.append_fills()) + 199                   # (the batch keeps at least 200 rows)
            elif c.op == "graph_search":
                last = max(C.window(C.VIEWS[c.view], ln).hi for ln in c.lines) - 1
            else:
                last = C.windows(v)[-1].hi - 1
            assert _offset(v, last, line) >= value, (c, line)
    # the table's b32 column: every store but the 2.1 GB of fp8 codes written for X16 has one
    assert {c.view for c in C.CASES if c.view and C.B32 not in c.lines} == {"q8_e128"}
    for line, fill in C.append_fills():
        rows = C.APPEND_ROWS[0] * C.APPEND_ROWS[1]
        first = C.window(C.VIEWS["x16_e128"], line).first
        assert fill < first < fill + 200 <= fill + rows and fill + rows + 64 <= C.N16
    b, e = C.maxsim_docs(C.VIEWS["x16_e768"])
    assert (e - b).max() == 70 and (e - b).min() == 0 and (b >= 0).all() and e.max() == C.VIEWS["x16_e768"].rows
    for name in ("x16_e128", "x16_e768", "c8_e128", "c8_e768"):
        v = C.VIEWS[name]
        b, e = C.maxsim_docs(v)
        big = set(C.compact_rows(C.windows(v)).tolist())
        assert all(r in big for lo, hi in zip(b, e) for r in range(lo, hi))         # the documents lie inside the windows
        for w in C.windows(v):
            for line in w.lines:
                value, u = C.LINE_VALUE[line], C.row_unit(v, line)
                inside = (b >= w.lo) & (e <= w.hi) & (e > b)
                assert ((e[inside] - 1) * u < value).any() and ((b[inside] * u < value) & ((e[inside] - 1) * u >= value)).any() \
                    and (b[inside] * u >= value).any(), (name, w)


def test_row_counts_are_inside_the_documented_limits():
    for c in C.CASES:
        limit = C.ROW_LIMIT[c.op]
        if c.view is not None and limit is not None:
            assert C.VIEWS[c.view].rows < limit, c
    assert set(C.ROW_LIMIT) == set(C.OPERATORS)
    g = C.GRAPH
    assert 1 <= g["k"] <= g["ef"] <= 2048 and 1 <= g["width"] <= 8 and 1 <= g["n_entry"] <= g["ef"] and g["M"] % 2 == 0
    assert 2 * (g["n_entry"] + g["iters_lds"] * g["width"] * g["M"]) <= 16384 < 2 * (g["n_entry"] + g["iters_ws"] * g["width"] * g["M"])
    assert C.KMEANS_NLIST <= 65536 and C.SEGMENT_NLIST <= 65536 and max(C.IVF_K) <= 4096 and C.IVF_NPROBE <= 4096
    assert C.APPEND_ROWS[0] * C.APPEND_ROWS[1] < 2 ** 31
    for op, cfg in C.FULL_SCAN.items():
        n = C.VIEWS[cfg["view"]].rows
        assert cfg["k"] <= 4096 and C.sample_m(cfg["k"], n) >= 4, op               # DESIGN §3.12's sampling envelope
    assert C.SEARCH["Q"] * C.SEARCH["k"] <= 16384 and C.SEARCH["row_shard"] % 64 == 0
    b, e = C.colbert_documents()
    T = 2 ** 31 - 1
    assert 200 <= b.size < 1000 and e.max() == T and b.min() == 0 and (e >= b).all()
    live = np.nonzero(e > b)[0]
    order = live[np.lexsort((e[live], b[live]))]
    assert (b[order][1:] >= e[order][:-1]).all()                                    # non-empty ranges are disjoint
    for at in (2 ** 24, 2 ** 30):
        assert ((e > b) & (e <= at) & (e > at - 200)).any() and ((e > b) & (b >= at) & (b < at + 200)).any()
    assert ((b >= T - 2 ** 8) & (e > b)).sum() > 20
    hits = C.colbert_hits(b, e)
    flat = set(hits.flatten().tolist())
    assert {T - 1, T, -1, 0} <= flat and set(b[live][:0].tolist()) <= flat and hits.shape[1] <= 16384
    assert len(flat & set(b[live].tolist())) > 20 and len(flat & set((e[live] - 1).tolist())) > 20


def test_workspaces_stay_under_two_gib(L):
    from matchmaker_amd import _lib
    sizes = {}
    for name, fn in (("x16_e128", L.mm_ivf_scan_workspace_bytes), ("x16_e768", L.mm_ivf_scan_workspace_bytes),
                     ("c8_e128", L.mm_ivf_scan_fp8_workspace_bytes), ("c8_e768", L.mm_ivf_scan_fp8_workspace_bytes),
                     ("c8_ah768", L.mm_ah_scan_workspace_bytes)):
        v = C.VIEWS[name]
        nlist = len(C.list_layout(v).begin_big) - 1
        for nq in C.IVF_NQ:
            for k in C.IVF_K:
                sizes[(name, nq, k)] = int(fn(v.rows, nlist, nq, C.IVF_NPROBE, k))
    assert max(sizes.values()) >= 2 ** 30                                           # (the candidate buffer reaches its 1 GiB cap)
    g = C.GRAPH
    for it in (g["iters_lds"], g["iters_ws"]):
        sizes[("graph", it)] = int(L.mm_graph_search_workspace_bytes(C.N16, g["nq"], g["M"], g["ef"], g["width"], g["n_entry"], it))
    assert sizes[("graph", g["iters_lds"])] == 256 < sizes[("graph", g["iters_ws"])]
    sizes["segment_sum"] = int(L.mm_kmeans_segment_sum_workspace_bytes(C.N16, C.SEGMENT_NLIST, C.E))
    for op, fn in (("dot_topk", L.mm_dot_topk_workspace_bytes), ("dot_topk_fp8", L.mm_dot_topk_fp8_workspace_bytes)):
        cfg = C.FULL_SCAN[op]
        sizes[op] = int(fn(C.VIEWS[cfg["view"]].rows, cfg["nq"], cfg["k"]))
        s = C.SEARCH
        sizes[op + " shard"] = int(fn(s["row_shard"], s["nq"] * s["Q"], s["k"]))
    sizes["store_append"] = int(L.mm_store_append_workspace_bytes(*C.APPEND_ROWS))
    sizes["colbert_candidates"] = int(L.mm_colbert_candidates_workspace_bytes(4, 96))
    for key, b in sizes.items():
        assert 0 < b < 2 ** 31, (key, b)
    for name in ("x16_e768", "c8_e768"):
        nb = C.maxsim_docs(C.VIEWS[name])[0].size
        for fn in (L.mm_maxsim_ragged_workspace_bytes, L.mm_maxsim_ragged_fp8_workspace_bytes):
            assert 0 <= int(fn(nb, C.MAXSIM_PAIRS_PER_QUERY, C.MAXSIM_Q, _lib.MASK_U8)) < 2 ** 31


def test_the_value_set_is_exact_at_both_widths():
    for width in (C.E, C.WIDE):
        assert C.exact_bound(width, scaled=False) < C.EXACT_LIMIT
        assert C.exact_bound(width, scaled=True) < C.EXACT_LIMIT                    # in the unit 2^-3 / 16 of the smallest scale
    assert C.exact_bound(C.WIDE, True) == 768 * 4 * 64
    # a MaxSim sum of Q such maxima, and an ah_scan score (a probe score of the same unit added last)
    assert C.MAXSIM_Q * C.exact_bound(C.WIDE, True) < C.EXACT_LIMIT and C.exact_bound(C.WIDE, False) + 64 < C.EXACT_LIMIT
    # kmeans_segment_sum: a list's column sum, in the unit 1 / VALUE_DEN
    lb = C.segment_list_begin()
    assert lb[0] == 0 and lb[-1] == C.N16 and (np.diff(lb) >= 0).all() and (np.diff(lb) == 0).sum() >= 20
    assert int(np.diff(lb).max()) * max(C.VALUE_NUM) < C.EXACT_LIMIT
    # every value is exact in float16, bfloat16 and e4m3fn, and no byte of C8 is one of e4m3fn's NaN patterns
    import torch
    vals = torch.tensor(C.VALUE_NUM, dtype=torch.float32) / C.VALUE_DEN
    for dt in (torch.float16, torch.bfloat16, torch.float8_e4m3fn):
        assert torch.equal(vals.to(dt).to(torch.float32), vals)
    codes = vals.to(torch.float8_e4m3fn).view(torch.uint8)
    assert ((codes & 0x7f) != 0x7f).all()
    # fp8_quantize_rows of an X16 row is exact: the row maximum is 1/4 or 1/2, the scaled values are 0, +-64, +-128 (or 256)
    from tests import fp8_store_reference as F
    x = (np.array([[-2, -1, 0, 1, 2], [-1, 0, 1, 1, 0], [0, 0, 0, 0, 0]]) / C.VALUE_DEN).astype(np.float32)
    codes, scales = F.quantize_numpy(x)
    assert np.array_equal(F.dequantize_numpy(codes, scales), x.astype(np.float64))


def test_entry_points_refuse_the_first_row_count_past_their_limit(L):
    """include/mm_native.h gives mm_dot_topk_fwd, mm_ivf_scan_fwd and mm_kmeans_segment_sum a 2^31 - 1 row limit that no CPU
    test asserted (the fp8, AH, graph, assignment and candidate entry points have theirs in their own modules)."""
    from matchmaker_amd import _lib
    p, big = 4096, 1 << 40                             # any non-null aligned value: refused before it is used
    F16 = _lib.MM_F16

    def dot(n):
        return L.mm_dot_topk_fwd(p, p, n, 2, 128, F16, 10, 1.0, p, p, p, p, big, None)

    def ivf(n):
        return L.mm_ivf_scan_fwd(p, p, p, p, n, 3, 1, 2, 128, F16, 2, p, p, p, big, None)

    def seg(n):
        return L.mm_kmeans_segment_sum(p, p, p, n, 3, 128, F16, p, p, big, None)

    for call in (dot, ivf, seg):
        assert call(1 << 31) == _lib.MM_EUNSUPPORTED, call.__name__
        assert b"2^31" in L.mm_last_error()
        assert call((1 << 40) + 5) == _lib.MM_EUNSUPPORTED, call.__name__
    assert L.mm_dot_topk_workspace_bytes((1 << 31) - 1, 2, 10) > 0 and L.mm_ivf_scan_workspace_bytes((1 << 31) - 1, 3, 1, 2, 2) > 0
    # one workgroup per 16 rows: the header now states the limits the host has always refused past
    assert L.mm_ah_encode(p, p, p, p, C.ROW_LIMIT["ah_encode"], 3, 128, F16, 1.0, 2, p, None) == _lib.MM_EUNSUPPORTED
    assert b"2^35" in L.mm_last_error()
    assert L.mm_fp8_quantize_rows(p, C.ROW_LIMIT["fp8_quantize_rows"], 128, F16, p, p, None) == _lib.MM_EUNSUPPORTED
    assert b"2^35 - 16" in L.mm_last_error()
    from tests import abi
    with open(os.path.join(abi.INCLUDE, "mm_native.h")) as f:
        hdr = f.read()
    assert "n_rows <= 2^35 - 16" in hdr and "n < 2^35" in hdr
