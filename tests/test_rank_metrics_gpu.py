"""GPU: the ranking and metric kernels of rank_metrics.hip (mm_segment_rank_fwd, mm_rank_metrics_fwd,
mm_rank_metrics_depth_fwd) through matchmaker_amd.ops and matchmaker_amd.metrics.EvalSet, against the row-by-row restatement
(tests/rank_metrics_reference.py) and against what the real core_metrics.py functions returned (tests/golden/rank_metrics_*).
Integers, RR and recall are compared exactly; AP and nDCG within 2 (m + 1) 2^-53 |want| (derivation: the restatement's
docstring).  Nothing is masked out of a comparison: NaN must meet NaN."""
import numpy as np
import pytest
import torch

from tests import rank_metrics_reference as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from matchmaker_amd import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.mm_native.*)
    return ops


def _same(a, b):
    """Dict equality where NaN meets NaN."""
    return list(a) == list(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def _segments(lengths):
    sb = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=sb[1:])
    return sb


def _check_order(order, want, sb):
    assert order.dtype == torch.int32
    got = order.cpu().numpy()
    for s in range(len(sb) - 1):                                 # a permutation of each segment
        assert np.array_equal(np.sort(got[sb[s]:sb[s + 1]]), np.arange(sb[s], sb[s + 1])), s
    assert np.array_equal(got, want)


# ---- ranking ---------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 0, 1, 2, 63, 0, 64, 65, 1000, 0, 1025, 8192, 3, 0]     # empty segments at the start, in the middle, at the end


@pytest.fixture(scope="module")
def mixed():
    ops = _ops()
    assert ops.RANK_MAX_LEN == 8192 == max(LENGTHS)
    sb = _segments(LENGTHS)
    rng = np.random.default_rng(0)
    n = int(sb[-1])
    kinds = {
        "equal": np.full(n, 0.25, np.float32),                                                 # pure stability
        "five": rng.integers(0, 5, n).astype(np.float32) - 2,                                  # many ties
        "random": rng.standard_normal(n).astype(np.float32),
        "negative": -np.abs(rng.standard_normal(n)).astype(np.float32) - 1,                    # every segment all-negative
        "special": rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 1.0, -1.0, 3e38], np.float32), n),
    }
    return sb, kinds, {k: RR.rank_ref(v, sb) for k, v in kinds.items()}


@pytest.mark.parametrize("kind", ["equal", "five", "random", "negative", "special"])
def test_segment_rank_is_the_stable_descending_sort(mixed, kind):
    sb, kinds, want = mixed
    ops = _ops()
    s = torch.from_numpy(kinds[kind]).to(DEV)
    sbt = torch.from_numpy(sb).to(DEV)
    order = ops.segment_rank(s, sbt, max(LENGTHS))
    _check_order(order, want[kind], sb)
    assert torch.equal(order, ops.segment_rank(s, sbt, max(LENGTHS)))            # two calls: the same bits
    assert torch.equal(order, torch.ops.mm_native.segment_rank(s, sbt, max(LENGTHS)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_segment_rank_widens_16_bit_scores_exactly(mixed, dtype):
    sb, kinds, _ = mixed
    s = torch.from_numpy(kinds["special"] * np.float32(0.5) + kinds["five"]).to(DEV).to(dtype)      # rounding creates more ties
    want = RR.rank_ref(s.float().cpu().numpy(), sb)
    _check_order(_ops().segment_rank(s, torch.from_numpy(sb).to(DEV), max(LENGTHS)), want, sb)


def test_segment_rank_small_bounds_and_empty_calls():
    """max_len <= 64 launches the wavefront kernel alone; nq = 0 and N = 0 succeed; nothing outside [0, N) is touched when
    seg_begin lies (the kernel clamps): the rows seg_begin does not cover keep what they held."""
    ops = _ops()
    rng = np.random.default_rng(1)
    lengths = [64, 0, 7, 1, 33, 64, 2]
    sb = _segments(lengths)
    sc = rng.integers(0, 4, int(sb[-1])).astype(np.float32)
    _check_order(ops.segment_rank(torch.from_numpy(sc).to(DEV), torch.from_numpy(sb).to(DEV), 64), RR.rank_ref(sc, sb), sb)
    empty = ops.segment_rank(torch.zeros(0, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 0)
    assert empty.numel() == 0
    assert ops.segment_rank(torch.zeros(0, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), 5).numel() == 0
    wild = torch.tensor([-5, 3, 3, 10 ** 12, 7], dtype=torch.int64, device=DEV)   # clamped to [0,3) [3,3) [3,10) [10,10)
    s = torch.tensor([1.0, 3.0, 2.0, 0.0, 5.0, 4.0, 9.0, 8.0, 7.0, 6.0], device=DEV)
    got = ops.segment_rank(s, wild, 16).cpu().numpy()
    assert np.array_equal(got, [1, 2, 0, 6, 7, 8, 9, 4, 5, 3])


def test_segment_rank_refuses_a_longer_bound_and_evalset_takes_the_numpy_route():
    from matchmaker_amd import _lib
    from matchmaker_amd.metrics import EvalSet
    ops = _ops()
    n = ops.RANK_MAX_LEN + 1
    s = torch.arange(n, dtype=torch.float32, device=DEV) % 7
    with pytest.raises(ops.NativeError) as e:
        ops.segment_rank(s, torch.tensor([0, n], dtype=torch.int64, device=DEV), n)
    assert e.value.code == _lib.MM_EUNSUPPORTED
    rc = _lib.lib().mm_segment_rank_fwd(s.data_ptr(), _lib.MM_F32, s.data_ptr(), n, 1, n, s.data_ptr(), None)   # before any launch
    assert rc == _lib.MM_EUNSUPPORTED and b"8192" in _lib.lib().mm_last_error()
    es = EvalSet(["q"] * n, [f"d{i}" for i in range(n)], {"q": {"d5": 1, "d6": 2}}).to(DEV)
    assert es.max_len == n
    order = es.rank(s)
    assert order.is_cuda and np.array_equal(order.cpu().numpy(), RR.rank_ref(s.cpu().numpy(), np.array([0, n])))
    with pytest.raises(ops.NativeError):
        es.rank(s, native=True)
    got = es.metrics_plain(s)
    want = es.metrics_plain(s.cpu(), native=False)
    assert _same(got, want) and got["QueriesRanked"] == 1


# ---- metrics against the goldens and the restatement -------------------------------------------------------------------------
@pytest.fixture(scope="module", params=RR.CASES)
def case(request):
    js, arr = RR.load_case(request.param)
    es = RR.eval_set(request.param)
    esd = es.to(DEV)
    scores = torch.from_numpy(arr["scores"]).to(DEV)
    order = esd.rank(scores)
    h = es._host
    rest = (es.binarization_point, es.rcut, es.ncut, es.map_cut, h["bnr"], h["idcg"], h["log2"])
    return js, arr, es, esd, scores, order, rest, RR.matched_rows(es)


def test_ranked_result_is_the_references(case):
    js, arr, es, esd, scores, order, rest, m = case
    assert np.array_equal(order.cpu().numpy(), RR.rank_ref(arr["scores"], es._host["seg_begin"]))
    got = esd.ranked_result(scores)
    assert got == js["ranking"] and list(got) == list(js["ranking"])


def _check_form(case, tag, threshold, want_dict):
    js, arr, es, esd, scores, order, rest, m = case
    h = es._host
    pq = tuple(x.cpu().numpy() for x in esd.per_query(scores, threshold))
    ref = RR.metrics_ref(order.cpu().numpy(), h["seg_begin"], h["grade"], None if threshold is None else h["cand_pos"], threshold, *rest)
    assert np.array_equal(pq[0], ref[0]) and np.array_equal(pq[1], ref[1]), tag            # first_rank, hits: exact
    RR.assert_close(pq[2], ref[2], m, tag + " ap vs restatement")
    RR.assert_close(pq[3], ref[3], m[:, None], tag + " ndcg vs restatement")
    RR.assert_per_query(es, pq, arr[tag + "_rr"], arr[tag + "_ap"], arr[tag + "_recall"], arr[tag + "_ndcg"], m, tag)
    m_mean = int(m.max()) + es.n_queries
    got = esd.metrics_plain(scores) if threshold is None else esd.metrics_single_candidate_threshold(scores, threshold)
    RR.assert_dict(got, want_dict, m_mean, tag)
    RR.assert_dict(RR.dict_ref(*ref[:4], h["bnr"], es.evaluated_queries, es.rcut, es.ncut, es.map_cut), want_dict, m_mean, tag + " restatement")
    again = tuple(x.cpu().numpy() for x in esd.per_query(scores, threshold))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(pq, again)), "two calls: the same bits"


def test_metrics_plain(case):
    _check_form(case, "plain", None, case[0]["plain"])


def test_metrics_single_candidate_threshold(case):
    for t, want in case[0]["single"].items():
        _check_form(case, f"single{t}", int(t), want)


def test_edge_queries_have_the_stated_values():
    """The golden 'edges' case holds what it was built for (read off the real functions' per-query outputs)."""
    js, arr = RR.load_case("edges")
    qids = list(dict.fromkeys(js["query_ids"]))
    rr, ap, ndcg = arr["plain_rr"], arr["plain_ap"], arr["plain_ndcg"]
    at = qids.index
    assert rr[0, at("none")] == 0 and rr[0, at("r1")] == 1 and rr[0, at("r10")] == 0.1 and rr[0, at("r11")] == 0
    assert rr[1, at("r11")] == 1 / 11
    assert ap[at("r1000")] == 1 / 1000 and ap[at("r1001")] == 0 and rr[4, at("r1000")] == 1 / 1000 and rr[4, at("r1001")] == 0
    assert np.isnan(ndcg[:, at("all0")]).all() and not np.isnan(np.delete(ndcg, at("all0"), axis=1)).any()
    assert (ndcg[:, at("unjudged")] == 0).all()


def test_depth_sweep_against_goldens_restatement_and_the_other_forms(case):
    js, arr, es, esd, scores, order, rest, m = case
    ops = _ops()
    h = es._host
    t = esd.t
    m_mean = int(m.max()) + es.n_queries
    for entry in js["depth"]:
        lo, hi = entry["range"]
        want = arr[f"depth_{lo}_{hi}"]
        dev = tuple(x.cpu().numpy() for x in ops.rank_metrics_depth(order, t["seg_begin"], t["grade"], t["cand_pos"], hi, *rest[:4],
                                                                    t["bnr"], t["idcg"], t["log2"]))
        ref = RR.depth_ref(order.cpu().numpy(), h["seg_begin"], h["grade"], h["cand_pos"], hi, *rest)
        assert np.array_equal(dev[0], ref[0]) and np.array_equal(dev[1], ref[1])
        RR.assert_close(dev[2], ref[2], m[:, None], "depth ap")
        RR.assert_close(dev[3], ref[3], m[:, None, None], "depth ndcg")
        for th in sorted({1, lo, (lo + hi) // 2, hi}):                # the sweep at t IS the single-threshold kernel at t
            one = tuple(x.cpu().numpy() for x in esd.per_query(scores, th, order=order))
            for a, b in zip(dev, one):
                assert np.array_equal(a[:, th - 1], b, equal_nan=True), (th, "sweep vs single threshold")
        for chunk in (None, 1, 4):                                    # 4 splits 9 and 40 queries unevenly
            got = esd.metrics_along_candidate_depth(scores, (lo, hi), query_chunk=chunk)
            assert list(got) == list(range(lo, hi + 1))
            for i, th in enumerate(range(lo, hi + 1)):
                RR.assert_dict(got[th], dict(zip(entry["keys"], want[i])), m_mean, f"depth {lo}-{hi} t={th} chunk={chunk}")


def test_depth_equals_single_threshold_everywhere_and_plain_at_hi():
    """Every t of the sweep against the single-threshold kernel, bit for bit; with cand_pos a permutation of 1..n per query,
    t = hi admits every row: the plain result."""
    ops = _ops()
    rng = np.random.default_rng(7)
    lengths = [65, 1, 0, 40, 64, 17]
    sb = _segments(lengths)
    n, nq, hi = int(sb[-1]), len(lengths), 65
    sc = rng.integers(0, 6, n).astype(np.float32)
    grade = np.where(rng.random(n) < 0.2, rng.integers(0, 4, n), RR.NOT_JUDGED).astype(np.int32)
    cand = np.concatenate([rng.permutation(l) + 1 for l in lengths]).astype(np.int32)
    bnr = np.array([max(1, int((grade[sb[q]:sb[q + 1]] >= 1).sum())) for q in range(nq)], np.int32)
    rcut, ncut, map_cut = [1, 5, 10], [3, 10], 20
    lg = np.log2(1 + np.arange(0, 12))
    idcg = np.abs(rng.standard_normal((nq, 2))) + 1
    dv = lambda a: torch.from_numpy(a).to(DEV)
    order = ops.segment_rank(dv(sc), dv(sb), 65)
    args = (1.0, rcut, ncut, map_cut, dv(bnr), dv(idcg), dv(lg))
    sweep = ops.rank_metrics_depth(order, dv(sb), dv(grade), dv(cand), hi, *args)
    assert sweep[0].shape == (nq, hi) and sweep[1].shape == (nq, hi, 3) and sweep[3].shape == (nq, hi, 2)
    for th in range(1, hi + 1):
        one = ops.rank_metrics(order, dv(sb), dv(grade), dv(cand), th, *args)
        for a, b in zip(sweep, one):
            assert np.array_equal(a[:, th - 1].cpu().numpy(), b.cpu().numpy(), equal_nan=True), th
    plain = ops.rank_metrics(order, dv(sb), dv(grade), None, 2 ** 31 - 1, *args)
    for a, b in zip(sweep, plain):
        assert np.array_equal(a[:, hi - 1].cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    ref = RR.metrics_ref(order.cpu().numpy(), sb, grade, None, None, 1.0, rcut, ncut, map_cut, bnr, idcg, lg)
    assert np.array_equal(plain[0].cpu().numpy(), ref[0]) and np.array_equal(plain[1].cpu().numpy(), ref[1])


def test_long_lists_cross_the_wavefront_step_and_the_sweep_blocks():
    """1,000 + 300 + 257 rows with judged rows on both sides of every 64-row step (the wavefront kernel's carry) and hi = 1000
    (four 256-lane blocks per query in the sweep), against the restatement."""
    ops = _ops()
    rng = np.random.default_rng(9)
    lengths = [1000, 300, 257]
    sb = _segments(lengths)
    n, nq, hi = int(sb[-1]), 3, 1000
    sc = rng.standard_normal(n).astype(np.float32)
    grade = np.where(rng.random(n) < 0.1, rng.integers(0, 3, n), RR.NOT_JUDGED).astype(np.int32)
    grade[[63, 64, 127, 128, 999]] = 2
    cand = np.concatenate([rng.permutation(l) + 1 for l in lengths]).astype(np.int32)
    bnr = np.array([int((grade[sb[q]:sb[q + 1]] >= 1).sum()) for q in range(nq)], np.int32)
    rcut, ncut, map_cut = [10, 100, 1000], [10, 1000], 1000
    lg = np.log2(1 + np.arange(0, 1002))
    idcg = np.abs(rng.standard_normal((nq, 2))) + 1
    dv = lambda a: torch.from_numpy(a).to(DEV)
    order = ops.segment_rank(dv(sc), dv(sb), 1000)
    o = order.cpu().numpy()
    assert np.array_equal(o, RR.rank_ref(sc, sb))
    args = (1.0, rcut, ncut, map_cut, bnr, idcg, lg)
    dargs = (1.0, rcut, ncut, map_cut, dv(bnr), dv(idcg), dv(lg))
    for th, cp in ((None, None), (500, cand)):
        got = ops.rank_metrics(order, dv(sb), dv(grade), None if cp is None else dv(cp), 2 ** 31 - 1 if th is None else th, *dargs)
        ref = RR.metrics_ref(o, sb, grade, cp, th, *args)
        assert np.array_equal(got[0].cpu().numpy(), ref[0]) and np.array_equal(got[1].cpu().numpy(), ref[1])
        RR.assert_close(got[2].cpu().numpy(), ref[2], ref[4])
        RR.assert_close(got[3].cpu().numpy(), ref[3], ref[4][:, None])
    sweep = ops.rank_metrics_depth(order, dv(sb), dv(grade), dv(cand), hi, *dargs)
    for th in (1, 255, 256, 257, 512, 1000):
        ref = RR.metrics_ref(o, sb, grade, cand, th, *args)
        assert np.array_equal(sweep[0][:, th - 1].cpu().numpy(), ref[0]) and np.array_equal(sweep[1][:, th - 1].cpu().numpy(), ref[1])
        RR.assert_close(sweep[2][:, th - 1].cpu().numpy(), ref[2], ref[4])
        RR.assert_close(sweep[3][:, th - 1].cpu().numpy(), ref[3], ref[4][:, None])


# ---- capture and the end-to-end route ----------------------------------------------------------------------------------------
def test_rank_and_plain_metrics_capture_in_a_graph_and_replay_on_new_scores():
    js, arr = RR.load_case("graded")
    esd = RR.eval_set("graded").to(DEV)
    first = torch.from_numpy(arr["scores"]).to(DEV)
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up outside capture
        esd.per_query(static)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        order = esd.rank(static)
        out = esd.per_query(static, order=order)
    g.replay()
    torch.cuda.synchronize()
    assert _same(esd.metrics_from_per_query(*out), esd.metrics_plain(first))
    new = torch.from_numpy(np.random.default_rng(3).integers(0, 9, first.numel()).astype(np.float32)).to(DEV)
    static.copy_(new)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(order, esd.rank(new))
    eager = esd.per_query(new)
    assert all(torch.equal(a, b) or np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True) for a, b in zip(out, eager))
    assert _same(esd.metrics_from_per_query(*out), esd.metrics_plain(new))


def test_evaluate_to_metrics_matches_the_host_route():
    from matchmaker_amd import rerank
    from matchmaker_amd.metrics import EvalSet

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, query, document, use_fp16=True, output_secondary_output=False):
            s = document["input_ids"].float().sum(-1) - query["input_ids"].float().sum(-1)
            return (s, {}) if output_secondary_output else s

    gen = torch.Generator().manual_seed(3)
    batches, qids, dids = [], [], []
    for b in range(12):
        n = 5
        qid = [f"q{(b * n + i) % 9}" for i in range(n)]              # the rows of a query do not arrive next to each other
        did = [f"d{(b * n + i) % 23}" for i in range(n)]
        q = torch.randint(0, 3, (n, 4), generator=gen)
        d = torch.randint(0, 3, (n, 6), generator=gen)               # small range: plenty of exact ties
        batches.append({"query_tokens": {"input_ids": q}, "doc_tokens": {"input_ids": d}, "query_id": qid, "doc_id": did})
        qids += qid
        dids += did
    qrels = {f"q{i}": {f"d{(3 * i + j) % 23}": j % 3 for j in range(4)} for i in range(0, 9, 2)}
    model = Model().to(DEV)
    es = EvalSet(qids, dids, qrels).to(DEV)
    ranked, metrics = rerank.evaluate_to_metrics(model, batches, es, use_fp16=False)
    unrolled = rerank.evaluate_batches(model, batches, use_fp16=False)
    assert ranked == rerank.unrolled_to_ranked_result(unrolled) and list(ranked) == list(unrolled)
    scores = torch.tensor([s for rows in unrolled.values() for _, s in rows])
    flat = torch.cat([(b["doc_tokens"]["input_ids"].float().sum(-1) - b["query_tokens"]["input_ids"].float().sum(-1)) for b in batches])
    assert _same(metrics, es.metrics_plain(flat.to(DEV)))
    host = EvalSet(qids, dids, qrels).metrics_plain(flat)             # the numpy route on the same scores
    RR.assert_dict(metrics, host, 4 + es.n_queries)
    assert scores.numel() == flat.numel()
    with pytest.raises(ValueError):
        rerank.evaluate_to_metrics(model, batches[:-1], es, use_fp16=False)
