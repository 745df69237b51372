"""GPU: every operator that reads or writes a resident store, on stores past 2^31 elements and 4 GiB.

The two buffers, their views, the windows around the lines where 32-bit addressing breaks and the list / document layouts
come from tests/large_store_cases.py (tests/test_large_store_cases_cpu.py proves they cross the lines).  The data is exact
(every fp32 sum is the same in any order), so EVERY comparison in this module is an equality:

  (a) indexed operators     big store == compact copy of the windows == the numpy restatement of the compact problem
  (b) row-wise operators    one call over the whole buffer == calls on slices of 2^20 rows == the restatement on the windows
  (c) full scans            == the float64 products on the device, ordered by (score descending, row ascending)

A wrapped or truncated offset still lands inside the 4 GiB allocation: nothing faults, the call scores other rows.  The rows
a wrap would land on hold other random values (asserted on the device), so such a call cannot pass."""
import types

import numpy as np
import pytest
import torch

from tests import colbert_search_reference as CS
from tests import fp8_store_reference as F
from tests import graph_reference as GR
from tests import ivf_fp8_reference as IF
from tests import ivf_reference as IR
from tests import kmeans_reference as KR
from tests import large_store_cases as C
from tests import scann_reference as SR
from tests import store_writer_reference as SW
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stores():
    """X16, C8 / S8, built once; the neighbour table of graph_search on first use.  Everything is freed at teardown."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < C.MIN_FREE_BYTES:
        pytest.skip("needs 24 GB of free device memory (two 4 GiB stores, 4 GiB of neighbours, 6 GiB of append outputs)")
    torch.cuda.reset_peak_memory_stats(dev)
    s = types.SimpleNamespace(dev=dev, NBR=None, cache={})
    s.X16 = C.fill_x16(dev)
    s.C8, s.S8 = C.fill_c8(dev)
    yield s
    peak = torch.cuda.max_memory_allocated(dev)
    s.X16 = s.C8 = s.S8 = s.NBR = None
    s.cache.clear()
    ops.clear_workspaces()
    torch.cuda.empty_cache()
    print(f"\n[large store] peak device memory allocated: {peak / 2 ** 30:.2f} GiB")


# ---------------------------------------------------------------------------------------------- helpers
def _dv(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.cpu().numpy()


def _view(s, name):
    """the store tensor(s) of a view: X16 views -> tensor; C8 views -> (codes, scales of the view's first rows)"""
    v = C.VIEWS[name]
    if v.buffer == "X16":
        return s.X16.view(v.rows, v.row_elems)
    return s.C8.view(v.rows, v.row_bytes), s.S8[: v.rows]


def _compact(t, ws):
    return torch.cat([t[w.lo: w.hi] for w in ws])


def _assert_a_wrap_lands_on_other_data(buf, v, ws):
    """the bytes 2^31 and 2^32 below every window (where there are any) differ from the window's"""
    flat = buf.view(-1)
    per = flat.element_size()
    for w in ws:
        a, b = w.lo * v.row_bytes // per, w.hi * v.row_bytes // per
        for shift in (2 ** 31 // per, 2 ** 32 // per):
            if a - shift >= 0:
                assert not torch.equal(flat[a:b], flat[a - shift: b - shift]), (v.name, w.name, shift)


def _f64(t):
    return _np(t).astype(np.float64)


def _eq_scores_rows(got, ref_s, ref_r, what):
    s, r = got
    assert np.array_equal(_np(r), ref_r), (what, np.argwhere(_np(r) != ref_r)[:5])
    assert np.array_equal(_f64(s), ref_s), what


def _big_equals_compact(big, compact, ws, what):
    """scores identical, rows identical after shifting back"""
    assert torch.equal(big[0], compact[0]), what
    assert np.array_equal(C.to_compact(_np(big[1]), ws), _np(compact[1])), what
    for extra_b, extra_c in zip(big[2:], compact[2:]):
        assert torch.equal(extra_b, extra_c), what


def _queries(nq, width, seed, dev):
    q = C.small_values((nq, width), seed)
    return q, _dv(q, dev, torch.float16)


# ---------------------------------------------------------------------------------------------- the data
def test_the_stores_hold_the_exact_value_set(stores):
    s = stores
    assert s.X16.shape == (C.N16, C.E) and s.C8.shape == (C.N8, C.E) and s.S8.shape == (C.N8,)
    assert s.X16.numel() > 2 ** 31 and s.X16.numel() * 2 > 2 ** 32 and s.C8.numel() > 2 ** 32
    allowed = torch.tensor(C.VALUE_NUM, dtype=torch.float32, device=s.dev) / C.VALUE_DEN
    codes = allowed.to(torch.float8_e4m3fn).view(torch.uint8)
    scales = torch.tensor([2.0 ** k for k in range(C.SCALE_EXP[0], C.SCALE_EXP[1] + 1)], device=s.dev)
    for name in ("x16_e128", "c8_e128"):
        v = C.VIEWS[name]
        for w in C.windows(v):
            if v.buffer == "X16":
                assert torch.isin(s.X16[w.lo: w.hi].float(), allowed).all()
            else:
                assert torch.isin(s.C8[w.lo: w.hi], codes).all() and torch.isin(s.S8[w.lo: w.hi], scales).all()
                assert ((s.C8[w.lo: w.hi] & 0x7f) != 0x7f).all()                      # no NaN byte
    assert len(torch.unique(s.S8[: 1 << 16])) == 7 and len(torch.unique(s.X16[-(1 << 10):])) == 5
    for name, v in C.VIEWS.items():
        if v.buffer in ("X16", "C8"):
            _assert_a_wrap_lands_on_other_data(s.X16 if v.buffer == "X16" else s.C8, v, C.windows(v))


# ---------------------------------------------------------------------------------------------- (a) indexed operators
@pytest.mark.parametrize("k", C.IVF_K)
@pytest.mark.parametrize("nq", C.IVF_NQ)
@pytest.mark.parametrize("name", ["x16_e128", "x16_e768"])
def test_ivf_scan_across_the_lines(stores, name, nq, k):
    from matchmaker_amd import ops
    s, v = stores, C.VIEWS[name]
    lay = C.list_layout(v)
    X = _view(s, name)
    comp = _compact(X, lay.windows)
    qn, q = _queries(nq, v.row_elems, 100 + nq + k, s.dev)
    p = C.probes_for(lay, nq)
    small = ops.ivf_scan(q, comp, _dv(lay.begin_compact, s.dev), _dv(p, s.dev), k)
    big = ops.ivf_scan(q, X, _dv(lay.begin_big, s.dev), _dv(C.probes_to_big(lay, p), s.dev), k)
    _big_equals_compact(big, small, lay.windows, (name, nq, k))
    ref_s, ref_r = IR.ivf_scan(qn, _np(comp.float()), lay.begin_compact, p, k)
    _eq_scores_rows(small, ref_s, ref_r, (name, nq, k))
    if nq > 1 and k > 16:
        assert (ref_r[1, 16:] == -1).all() and (ref_r[1, :16] >= 0).all()             # k larger than the probed union


@pytest.mark.parametrize("k", C.IVF_K)
@pytest.mark.parametrize("nq", C.IVF_NQ)
@pytest.mark.parametrize("name", ["c8_e128", "c8_e768"])
def test_ivf_scan_fp8_across_the_lines(stores, name, nq, k):
    from matchmaker_amd import ops
    s, v = stores, C.VIEWS[name]
    lay = C.list_layout(v)
    codes, scales = _view(s, name)
    cc, sc = _compact(codes, lay.windows), _compact(scales, lay.windows)
    qn, q = _queries(nq, v.row_elems, 200 + nq + k, s.dev)
    p = C.probes_for(lay, nq)
    small = ops.ivf_scan_fp8(q, cc, sc, _dv(lay.begin_compact, s.dev), _dv(p, s.dev), k)
    big = ops.ivf_scan_fp8(q, codes, scales, _dv(lay.begin_big, s.dev), _dv(C.probes_to_big(lay, p), s.dev), k)
    _big_equals_compact(big, small, lay.windows, (name, nq, k))
    ref_s, ref_r = IF.ivf_scan_fp8(qn, _np(cc), _np(sc), lay.begin_compact, p, k)
    _eq_scores_rows(small, ref_s, ref_r, (name, nq, k))


@pytest.mark.parametrize("k", C.IVF_K)
@pytest.mark.parametrize("nq", C.IVF_NQ)
def test_ah_scan_across_the_lines(stores, nq, k):
    from matchmaker_amd import ops
    s, v = stores, C.VIEWS["c8_ah768"]
    lay = C.list_layout(v)
    codes = s.C8.view(v.rows, v.row_bytes)                                            # every byte is two valid 4-bit codes
    cc = _compact(codes, lay.windows)
    qn, q = _queries(nq, C.WIDE, 300 + nq + k, s.dev)
    cbn = C.small_values((C.WIDE // 2, 16, 2), 301)
    cb = _dv(cbn, s.dev, torch.float16)
    p = C.probes_for(lay, nq)
    psn = (np.random.default_rng(302).integers(-8, 9, p.shape) / 16.0).astype(np.float32)
    psn[psn == 0] = 0.0625                                                            # non-zero probe scores
    ps = _dv(psn, s.dev)
    small = ops.ah_scan(q, cc, cb, _dv(lay.begin_compact, s.dev), _dv(p, s.dev), ps, k)
    big = ops.ah_scan(q, codes, cb, _dv(lay.begin_big, s.dev), _dv(C.probes_to_big(lay, p), s.dev), ps, k)
    _big_equals_compact(big, small, lay.windows, (nq, k))
    ref_s, ref_r = SR.ah_scan(qn, _np(cc), cbn, lay.begin_compact, p, psn, k)
    _eq_scores_rows(small, ref_s, ref_r, (nq, k))


@pytest.mark.parametrize("name", ["x16_e128", "x16_e768"])
def test_gather_dot_across_the_lines(stores, name):
    from matchmaker_amd import ops
    s, v = stores, C.VIEWS[name]
    ws = C.windows(v)
    X = _view(s, name)
    comp = _compact(X, ws)
    nq, R = 6, C.GATHER_R
    qn, q = _queries(nq, v.row_elems, 400, s.dev)
    rows = C.to_big(np.random.default_rng(401).integers(0, comp.shape[0], (nq, R)), ws)
    edge = [w.lo for w in ws] + [w.hi - 1 for w in ws]                                # first and last row of every window
    line = [r for w in ws if w.lines for r in (w.first - 1, w.first)]                 # either side of every line
    rows[0, : len(edge)] = edge
    rows[1, : len(line)] = line
    rows[1, len(line):] = -1
    rows[2, 0], rows[2, R - 1] = v.rows - 1, -1                                       # the store's last row
    rows_c = C.to_compact(rows, ws)
    big = ops.gather_dot(q, X, _dv(rows, s.dev))
    small = ops.gather_dot(q, comp, _dv(rows_c, s.dev))
    assert torch.equal(big, small)
    assert np.array_equal(_f64(small), SR.gather_dot(qn, _np(comp.float()), rows_c))
    assert np.isneginf(_np(big)[1, len(line):]).all()


@pytest.mark.parametrize("line", [C.B31, C.B32])
def test_graph_search_across_the_lines(stores, line):
    """vectors AND the neighbour table ([N16, 64] int32: 256 bytes a row, as the vectors) cross the line at the same rows"""
    from matchmaker_amd import ops
    s, g = stores, C.GRAPH
    w = C.window(C.VIEWS["x16_e128"], line)
    assert w[1:3] == C.window(C.VIEWS["nbr_m64"], line)[1:3]                          # the same rows in both tables
    if s.NBR is None:
        s.NBR = torch.full((C.N16, g["M"]), -1, dtype=torch.int32, device=s.dev)
    comp = s.X16[w.lo: w.hi].clone()
    x = _np(comp.float())
    graph = GR.build(x, g["M"])
    gd = _dv(graph, s.dev)
    s.NBR[w.lo: w.hi] = torch.where(gd >= 0, gd + w.lo, gd)
    try:
        qn, q = _queries(g["nq"], C.E, 500, s.dev)
        e = np.random.default_rng(501).integers(0, x.shape[0], (g["nq"], g["n_entry"])).astype(np.int32)
        p = w.first - w.lo
        e[0, :4] = [p - 1, p, 0, x.shape[0] - 1]
        e[1, ::2] = -1
        eb = np.where(e >= 0, e + w.lo, e).astype(np.int32)
        for iters in (g["iters_lds"], g["iters_ws"]):                                 # the visited table in LDS / in the workspace
            small = ops.graph_search(q, comp, gd, _dv(e, s.dev), g["ef"], g["k"], g["width"], iters, return_stats=True)
            big = ops.graph_search(q, s.X16, s.NBR, _dv(eb, s.dev), g["ef"], g["k"], g["width"], iters, return_stats=True)
            assert torch.equal(big[0], small[0]) and torch.equal(big[2], small[2]), iters
            rb, rc = _np(big[1]), _np(small[1])
            assert np.array_equal(np.where(rb >= 0, rb - w.lo, rb), rc), iters
            rs, rr, it, sc = GR.search(x, graph, qn, e, g["ef"], g["width"], iters, g["k"])
            _eq_scores_rows(small[:2], rs, rr, iters)
            st = _np(small[2])
            assert np.array_equal(st[:, 0], it) and np.array_equal(st[:, 1], sc), iters
            assert (rb[rb >= 0] >= w.first).any() and (rb[rb >= 0] < w.first).any()   # results from both sides of the line
    finally:
        s.NBR[w.lo: w.hi] = -1


def _maxsim_case(s, name, run_big, run_small, codes_of):
    """shared by the 16-bit and the fp8 ragged MaxSim: documents of 1 .. 70 rows in, across and beyond every line"""
    v = C.VIEWS[name]
    ws = C.windows(v)
    b, e = C.maxsim_docs(v)
    bc = np.where(e > b, C.to_compact(np.minimum(b, v.rows - 1), ws), 0)
    ec = bc + (e - b)
    ppq, Q = C.MAXSIM_PAIRS_PER_QUERY, C.MAXSIM_Q
    nq = -(-b.size // ppq)
    qn = C.small_values((nq, Q, v.row_elems), 600)
    qn[:, 3] = 0                                                                      # a zero query row (scores 0 everywhere)
    q = _dv(qn, s.dev, torch.float16)
    mask = np.ones((nq, Q), dtype=bool)
    mask[:, Q // 2] = False
    mask[0, Q - 1] = False
    md = _dv(mask, s.dev)
    codes_c, scales_c = codes_of(ws)
    for sim_round, sum_round in ((False, False), (True, False), (True, True)):
        kw = dict(q_mask=md, pairs_per_query=ppq, sim_round=sim_round, sum_round=sum_round)
        big = run_big(q, _dv(b, s.dev), _dv(e, s.dev), **kw)
        small = run_small(q, _dv(bc, s.dev), _dv(ec, s.dev), **kw)
        assert torch.equal(big, small), (name, sim_round, sum_round)
        flags = (F.SIM_ROUND if sim_round else 0) | (F.SUM_ROUND if sum_round else 0)
        ref = F.maxsim_ragged_fp8_ref(qn, codes_c, scales_c, bc, ec, mask, ppq, flags, q_dtype=torch.float16)
        assert np.array_equal(_f64(small), ref), (name, sim_round, sum_round)
    assert (e == b).sum() >= 4


@pytest.mark.parametrize("name", ["x16_e128", "x16_e768"])
def test_maxsim_ragged_across_the_lines(stores, name):
    from matchmaker_amd import ops
    s = stores
    X = _view(s, name)
    comp = {}

    def codes_of(ws):
        """the compact 16-bit rows as e4m3fn codes with scale 1: the fp8 restatement then states the 16-bit operator"""
        comp["t"] = _compact(X, ws)
        c = _np(comp["t"].float().cpu().to(torch.float8_e4m3fn).view(torch.uint8))
        assert np.array_equal(F.deq_numpy(c), _f64(comp["t"]))
        return c, np.ones(c.shape[0], np.float32)

    _maxsim_case(s, name, lambda q, b, e, **kw: ops.maxsim_ragged(q, X, b, e, **kw),
                 lambda q, b, e, **kw: ops.maxsim_ragged(q, comp["t"], b, e, **kw), codes_of)


@pytest.mark.parametrize("name", ["c8_e128", "c8_e768"])
def test_maxsim_ragged_fp8_across_the_lines(stores, name):
    from matchmaker_amd import ops
    s = stores
    codes, scales = _view(s, name)
    comp = {}

    def codes_of(ws):
        comp["c"], comp["s"] = _compact(codes, ws), _compact(scales, ws)
        return _np(comp["c"]), _np(comp["s"])

    _maxsim_case(s, name, lambda q, b, e, **kw: ops.maxsim_ragged_fp8(q, codes, scales, b, e, **kw),
                 lambda q, b, e, **kw: ops.maxsim_ragged_fp8(q, comp["c"], comp["s"], b, e, **kw), codes_of)


def test_kmeans_segment_sum_over_the_whole_store(stores):
    from matchmaker_amd import ops
    s = stores
    g = torch.Generator(device=s.dev).manual_seed(700)
    order = torch.randperm(C.N16, generator=g, device=s.dev)
    lbn = C.segment_list_begin()
    lb = _dv(lbn, s.dev)
    got = ops.kmeans_segment_sum(s.X16, order, lb)
    list_of = torch.repeat_interleave(torch.arange(C.SEGMENT_NLIST, device=s.dev), lb[1:] - lb[:-1])
    # float64 index_add_ on exact data: order-free.  Every list gets 1,024 accumulator rows (position mod 1,024), summed
    # afterwards: 130 target rows alone would serialise 2 x 10^9 atomic additions
    sub = 1024
    slot = list_of * sub + torch.arange(C.N16, device=s.dev) % sub
    wide = torch.zeros(C.SEGMENT_NLIST * sub, C.E, dtype=torch.float64, device=s.dev)
    for lo in range(0, C.N16, C.CHUNK):
        hi = min(C.N16, lo + C.CHUNK)
        wide.index_add_(0, slot[lo:hi], s.X16[order[lo:hi]].double())
    ref = wide.view(C.SEGMENT_NLIST, sub, C.E).sum(dim=1)
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(got.view(torch.int32), ref.float().view(torch.int32))
    empty = np.nonzero(np.diff(lbn) == 0)[0]
    assert empty.size >= 20 and (got[_dv(empty, s.dev)] == 0).all() and (got != 0).any()
    # the restatement, on the three shortest lists that hold rows
    lens = np.diff(lbn)
    assert int(order.max()) == C.N16 - 1
    for l in np.argsort(np.where(lens > 0, lens, lens.max() + 1))[:3]:
        ordn = _np(order[lbn[l]: lbn[l + 1]])
        x = _np(s.X16[_dv(ordn, s.dev)].float())
        one = KR.segment_sum(x, np.arange(ordn.size), np.array([0, ordn.size]))
        assert np.array_equal(_f64(got[int(l)]), one[0])


# ---------------------------------------------------------------------------------------------- (b) row-wise operators
def _chunks(n):
    return [(lo, min(n, lo + C.CHUNK)) for lo in range(0, n, C.CHUNK)]


@pytest.mark.parametrize("name", ["x16_e128", "x16_e768"])
def test_kmeans_assign_whole_chunks_and_windows(stores, name):
    from matchmaker_amd import ops
    s, v = stores, C.VIEWS[name]
    X = _view(s, name)
    cn = C.small_values((C.KMEANS_NLIST, v.row_elems), 800)
    cent = _dv(cn, s.dev, torch.float16)
    lists, score = ops.kmeans_assign(X, cent)
    for lo, hi in _chunks(v.rows):                                                    # (a slice starts at offset 0 again)
        l1, s1 = ops.kmeans_assign(X[lo:hi], cent)
        assert torch.equal(lists[lo:hi], l1) and torch.equal(score[lo:hi], s1), (lo, hi)
    for w in C.windows(v):
        a, sc = KR.assign(_np(X[w.lo: w.hi].float()), cn)
        assert np.array_equal(_np(lists[w.lo: w.hi]).astype(np.int64), a), w
        assert np.array_equal(_f64(score[w.lo: w.hi]), sc), w
    assert len(torch.unique(lists)) == C.KMEANS_NLIST


def test_fp8_quantize_rows_whole_chunks_and_windows(stores):
    """2.1 GB of codes: the OUTPUT crosses 2^31 bytes at row 2^24, where the input crosses 2^32"""
    from matchmaker_amd import ops
    s, v = stores, C.VIEWS["x16_e128"]
    codes, scales = ops.fp8_quantize_rows(s.X16)
    assert codes.numel() > 2 ** 31
    for lo, hi in _chunks(C.N16):
        c1, s1 = ops.fp8_quantize_rows(s.X16[lo:hi])
        assert torch.equal(codes[lo:hi], c1) and torch.equal(scales[lo:hi], s1), (lo, hi)
    for w in C.windows(v) + C.windows(C.VIEWS["q8_e128"]):
        x = _np(s.X16[w.lo: w.hi].float())
        rc, rs = F.quantize_numpy(x)
        assert np.array_equal(_np(codes[w.lo: w.hi]), rc) and np.array_equal(_np(scales[w.lo: w.hi]), rs), w
        assert np.array_equal(F.dequantize_numpy(rc, rs), x.astype(np.float64))       # exact: the store's values survive


def _encode_problem(s, n):
    """centres = odd multiples of 1/8 up to 3/8, every block's codebook the grid {-1.5, -0.5, 0.5, 1.5}^2 in a seeded order
    (tests/scann_reference.py's exact store): a residual of a multiple of 1/4 never sits half-way between two codewords"""
    rng = np.random.default_rng(900)
    cn = (rng.choice([-3, -1, 1, 3], (C.KMEANS_NLIST, C.WIDE)) / 8.0).astype(np.float32)
    grid = np.array([(a, b) for a in (-1.5, -0.5, 0.5, 1.5) for b in (-1.5, -0.5, 0.5, 1.5)], np.float32)
    cbn = np.stack([grid[rng.permutation(16)] for _ in range(C.WIDE // 2)])
    g = torch.Generator(device=s.dev).manual_seed(901)
    lists = torch.randint(0, C.KMEANS_NLIST, (n,), generator=g, device=s.dev, dtype=torch.int32)
    return cn, cbn, lists


def test_ah_encode_whole_chunks_and_windows(stores):
    from matchmaker_amd import ops
    s, v = stores, C.VIEWS["x16_e768"]
    X = _view(s, "x16_e768")
    cn, cbn, lists = _encode_problem(s, v.rows)
    ws = C.windows(v)
    for w in ws:                                                                      # leaves outside [0, nlist): a zero centre
        lists[w.lo + 5], lists[w.hi - 1] = -1, C.KMEANS_NLIST
    cent, cb = _dv(cn, s.dev, torch.float16), _dv(cbn, s.dev, torch.float16)
    eta_real = (C.WIDE - 1) * 0.04 / 0.96                                             # tests/test_scann_gpu.py's eta_of(768)
    for eta in (1.0, eta_real):
        codes = ops.ah_encode(X, lists, cent, cb, eta, 2)
        assert codes.shape == (v.rows, C.AH_BYTES)
        for lo, hi in _chunks(v.rows):
            assert torch.equal(codes[lo:hi], ops.ah_encode(X[lo:hi], lists[lo:hi], cent, cb, eta, 2)), (eta, lo, hi)
        if eta != 1.0:
            continue
        # eta = 1: the cost is the plain distance, every fp32 step of the restatement is exact on this data
        for w in ws:
            lo, hi = (w.first - 150, w.first + 150) if w.lines else ((w.lo, w.lo + 300) if w.lo == 0 else (w.hi - 300, w.hi))
            ref = SR.encode(_np(X[lo:hi].float()), _np(lists[lo:hi]), cn, cbn, 1.0, 2)
            assert np.array_equal(_np(codes[lo:hi]), ref), w


def test_store_append_across_the_lines(stores):
    """rows_out [N16, 128] float16 reaches 2^31 bytes at row 2^23 and 2^32 at 2^24; codes_out reaches 2^31 at 2^24"""
    from matchmaker_amd import ops
    s = stores
    cap = C.N16
    rows_out = torch.empty(cap, C.E, dtype=torch.float16, device=s.dev)
    codes_out = torch.empty(cap, C.E, dtype=torch.uint8, device=s.dev)
    scales_out = torch.empty(cap, dtype=torch.float32, device=s.dev)
    n_docs, D = C.APPEND_ROWS
    xn = C.small_values((n_docs, D, C.E), 1000)
    xn[2] = 0                                                                         # an empty document
    xn[:, 5] = 0                                                                      # all-zero rows inside documents
    xn[4, 30:] = 0                                                                    # zero padding behind a short one
    x_cpu = torch.from_numpy(xn).to(torch.float16)
    x = x_cpu.to(s.dev)
    for line, fill0 in C.append_fills():
        want_rows, want_b, want_e = SW.append_batches([(x_cpu, False)], fill0)
        kept = want_rows.shape[0]
        first = C.window(C.VIEWS["x16_e128"], line).first
        assert 200 <= kept < n_docs * D and fill0 < first < fill0 + kept and (want_e == want_b).any()
        lo, hi = fill0 - 64, fill0 + kept + 64
        rows_out[lo:hi], codes_out[lo:hi], scales_out[lo:hi] = 7.0, 0x55, 3.0         # a pattern under and around the window
        fill = torch.tensor([fill0], dtype=torch.int64, device=s.dev)
        status = torch.zeros(1, dtype=torch.int32, device=s.dev)
        db = torch.full((n_docs,), -5, dtype=torch.int64, device=s.dev)
        de = torch.full((n_docs,), -5, dtype=torch.int64, device=s.dev)
        ops.store_append(x, rows_out, codes_out, scales_out, cap, fill, db, de, status)
        assert int(status[0]) == 0 and int(fill[0]) == fill0 + kept
        assert np.array_equal(_np(db), want_b) and np.array_equal(_np(de), want_e)
        assert torch.equal(SW.bits(rows_out[fill0: fill0 + kept].cpu()), SW.bits(want_rows)), line
        wc, wsc = F.quantize_torch(want_rows)
        assert torch.equal(codes_out[fill0: fill0 + kept].cpu(), wc) and torch.equal(scales_out[fill0: fill0 + kept].cpu(), wsc)
        for a, b in ((lo, fill0), (fill0 + kept, hi)):                                # 64 rows either side: untouched
            assert (rows_out[a:b] == 7.0).all() and (codes_out[a:b] == 0x55).all() and (scales_out[a:b] == 3.0).all(), line


def test_colbert_candidates_at_rows_up_to_two_to_the_31(stores):
    from matchmaker_amd import ops
    s = stores
    T = 2 ** 31 - 1
    b, e = C.colbert_documents(T)
    hits = C.colbert_hits(b, e, T)
    bs, es, ds = CS.sorted_view(b, e)
    c_cap = min(hits.shape[1], bs.size)
    got = ops.colbert_candidates(_dv(hits, s.dev), _dv(bs, s.dev), _dv(es, s.dev), _dv(ds, s.dev), T, c_cap)
    cands = CS.candidates_ref(hits, b, e)
    ref = CS.padded_candidates(cands, b, e, c_cap)
    for g, r in zip(got, ref):
        assert np.array_equal(_np(g), r)
    owner_of_last = [d for d in range(b.size) if b[d] <= T - 1 < e[d]]
    assert len(owner_of_last) == 1 and owner_of_last[0] in cands[0]                   # the hit at T - 1 found its owner
    assert max(len(c) for c in cands) > 40 and (ref[2] >= 2 ** 31 - 2 ** 8).any() and (ref[1] > 2 ** 30).any()


# ---------------------------------------------------------------------------------------------- (c) full scans
def _topk_f64(full, k):
    """the k best of a float64 score matrix on the device by (score descending, row ascending): a stable sort of the
    negated scores (torch.topk leaves the order of equal scores open)"""
    order = torch.sort(-full, dim=1, stable=True).indices[:, :k]
    return torch.gather(full, 1, order), order


def _scores_f64(q, rows_of, n, slab=1 << 18):
    """[nq, n] float64 on the device: the products in slabs of 2^18 rows; rows_of(lo, hi) -> float64 [hi - lo, E]"""
    full = torch.empty(q.shape[0], n, dtype=torch.float64, device=q.device)
    qd = q.double()
    for lo in range(0, n, slab):
        hi = min(n, lo + slab)
        full[:, lo:hi] = qd @ rows_of(lo, hi).T
    return full


def _planted_rows(v):
    """the first row, the row that straddles 2^32 bytes, the row after it, the last row"""
    first = C.window(v, C.B32).first
    assert (first - 1) * v.row_bytes < 2 ** 32 < first * v.row_bytes                  # (a row straddles it at E = 768)
    return [0, first - 1, first, v.rows - 1]


PLANT_SCALES = (3.0, 2.5, 2.0, 2.0)        # the last two tie: the lower row leads


def test_dot_topk_over_the_768_wide_view(stores):
    from matchmaker_amd import ops
    s, cfg = stores, C.FULL_SCAN["dot_topk"]
    v = C.VIEWS[cfg["view"]]
    X = _view(s, cfg["view"])
    qn, q = _queries(cfg["nq"], C.WIDE, 1100, s.dev)
    rows = _dv(np.array(_planted_rows(v)), s.dev)
    saved = X[rows].clone()
    try:
        X[rows] = (q[0].float()[None, :] * torch.tensor(PLANT_SCALES, device=s.dev)[:, None]).half()
        assert torch.equal(X[rows].float(), q[0].float()[None, :] * torch.tensor(PLANT_SCALES, device=s.dev)[:, None])
        got_s, got_i = ops.dot_topk(q, X, cfg["k"])
        full = _scores_f64(q, lambda lo, hi: X[lo:hi].double(), v.rows)
        ref_s, ref_i = _topk_f64(full, cfg["k"])
        assert torch.equal(got_i, ref_i) and torch.equal(got_s.double(), ref_s)
        assert got_i[0, :4].tolist() == _planted_rows(v)
    finally:
        X[rows] = saved


def test_dot_topk_fp8_over_the_768_wide_view(stores):
    from matchmaker_amd import ops
    s, cfg = stores, C.FULL_SCAN["dot_topk_fp8"]
    v = C.VIEWS[cfg["view"]]
    codes, scales = _view(s, cfg["view"])
    qn, q = _queries(cfg["nq"], C.WIDE, 1200, s.dev)
    rows = _dv(np.array(_planted_rows(v)), s.dev)
    saved_c, saved_s = codes[rows].clone(), scales[rows].clone()
    try:
        planted = q[0].float()[None, :] * torch.tensor(PLANT_SCALES, device=s.dev)[:, None]
        codes[rows] = planted.to(torch.float8_e4m3fn).view(torch.uint8)
        scales[rows] = 1.0
        assert torch.equal(codes[rows].view(torch.float8_e4m3fn).float(), planted)
        got_s, got_i = ops.dot_topk_fp8(q, codes, scales, cfg["k"])
        full = _scores_f64(q, lambda lo, hi: codes[lo:hi].view(torch.float8_e4m3fn).float().double() * scales[lo:hi].double()[:, None],
                           v.rows)
        ref_s, ref_i = _topk_f64(full, cfg["k"])
        assert torch.equal(got_i, ref_i) and torch.equal(got_s.double(), ref_s)
        assert got_i[0, :4].tolist() == _planted_rows(v)
    finally:
        codes[rows], scales[rows] = saved_c, saved_s


def _documents(n):
    """lengths cycling through 1 .. 127 until every one of the n rows has an owner"""
    per = 127 * 128 // 2
    lens = np.tile(np.arange(1, 128), n // per + 1)
    end = np.cumsum(lens)
    cut = int(np.searchsorted(end, n))
    end = end[: cut + 1].copy()
    end[-1] = n
    begin = np.concatenate([[0], end[:-1]])
    return begin.astype(np.int64), end.astype(np.int64)


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16", "fp8"])
def test_sharded_token_search_and_ranking_over_all_rows(stores, fp8):
    """TokenStore over all 16.8 M rows of X16: token_hits in shards of 2^20 rows == the float64 reference; rank_hits == the same
    call on a compact store of the candidate documents == the numpy restatement.  fp8: the store quantised by quantize_fp8()
    (exact on this data), searched with token_search="fp8".  Only 6,002 rows lie past 2^24, so every query's live tokens are
    planted, doubled, into a document there: the last shard, the candidate stage and the MaxSim all have to reach it."""
    from matchmaker_amd.token_store import TokenStore
    s, cfg = stores, C.SEARCH
    begin, end = _documents(C.N16)
    assert begin.size > 260000 and end[-1] == C.N16 and (end - begin).max() == 127
    qn = C.small_values((cfg["nq"], cfg["Q"], C.E), 1300)
    rng = np.random.default_rng(1301)
    for i in range(cfg["nq"]):
        qn[i, rng.choice(cfg["Q"], 2, replace=False)] = 0                             # two dead tokens per query
    q = _dv(qn, s.dev, torch.float16)
    flat = q.view(-1, C.E)
    live = torch.nonzero((flat != 0).any(dim=1)).flatten()
    n_live = cfg["Q"] - 2
    assert live.numel() == cfg["nq"] * n_live
    tail_docs = np.nonzero((begin >= 2 ** 24) & (end - begin >= n_live))[0][-cfg["nq"]:]
    assert tail_docs.size == cfg["nq"]
    planted = _dv(np.concatenate([np.arange(begin[d], begin[d] + n_live) for d in tail_docs]), s.dev)
    saved = s.X16[planted].clone()
    try:
        s.X16[planted] = flat[live] * 2                                               # query i's tokens -> document tail_docs[i]
        store = TokenStore(s.X16, range(begin.size), begin, end)
        kw = {}
        if fp8:
            store = store.quantize_fp8()
            kw = dict(token_search="fp8")
            for w in C.windows(C.VIEWS["q8_e128"]):                                   # the codes state the same values
                assert torch.equal(F.dequantize_torch(store.codes[w.lo: w.hi], store.scales[w.lo: w.hi], torch.float16),
                                   s.X16[w.lo: w.hi])
        hits = store.token_hits(q, cfg["k"], row_shard=cfg["row_shard"], **kw)
        if "token hits" not in s.cache:                                               # one reference for both stores
            want = torch.full((flat.shape[0], cfg["k"]), -1, dtype=torch.int64, device=s.dev)
            for a in range(0, live.numel(), 6):
                sel = live[a: a + 6]
                want[sel] = _topk_f64(_scores_f64(flat[sel], lambda lo, hi: s.X16[lo:hi].double(), C.N16), cfg["k"])[1]
            s.cache["token hits"] = want
        want = s.cache["token hits"]
        assert torch.equal(hits, want.view(cfg["nq"], -1))
        assert torch.equal(want[live][:, 0], planted)                                 # every live token found its planted row first
        assert ((hits >= 0) & (hits < 2 ** 23)).any() and ((hits >= 2 ** 23) & (hits < 2 ** 24)).any()
        # the candidates' rows as a compact store
        hn = _np(hits)
        docs = np.unique(np.searchsorted(end, hn[hn >= 0], side="right"))
        assert np.isin(tail_docs, docs).all()
        lens = (end - begin)[docs]
        ec = np.cumsum(lens)
        bc = ec - lens
        doc_of_hit = np.searchsorted(end, np.maximum(hn, 0), side="right")
        slot = np.minimum(np.searchsorted(docs, doc_of_hit), docs.size - 1)
        hc = np.where(hn >= 0, hn - begin[doc_of_hit] + bc[slot], -1)
        pick = _dv(np.concatenate([np.arange(begin[d], end[d]) for d in docs]), s.dev)
        small = TokenStore(s.X16[pick], range(docs.size), bc, ec)
        if fp8:
            small = small.quantize_fp8()
        big_s, big_i = store.rank_hits(q, hits, cfg["top_n"])
        small_s, small_i = small.rank_hits(q, _dv(hc, s.dev), cfg["top_n"])
        assert torch.equal(big_s, small_s)
        si = _np(small_i)
        assert (si >= 0).all()
        assert np.array_equal(_np(big_i), docs[si])
        assert np.array_equal(_np(big_i)[:, 0], tail_docs)                            # the planted document past 2^24 leads
        ref_s, ref_i, _ = CS.search_ref(qn, _np(s.X16[pick].float()), bc, ec, cfg["k"], cfg["top_n"], True, hit_rows=hc)
        assert np.array_equal(_np(small_s), ref_s) and np.array_equal(si, ref_i)
    finally:
        s.X16[planted] = saved
