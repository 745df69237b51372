"""CPU: the host side of the ranking / metrics feature.  The row-by-row restatement (tests/rank_metrics_reference.py) and
matchmaker_amd.metrics' numpy route against the recorded outputs of the real core_metrics.py functions (tests/golden) and,
where the reference tree is mounted, against the functions themselves; EvalSet's join; the C header, the binding, the
refusals that come before any launch, and the fake rule of torch.ops.mm_native.segment_rank."""
import importlib.util
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import rank_metrics_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mm_segment_rank_fwd", "mm_rank_metrics_fwd", "mm_rank_metrics_depth_fwd")


def _same(a, b):
    return list(a) == list(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


@pytest.fixture(scope="module", params=RR.CASES)
def case(request):
    js, arr = RR.load_case(request.param)
    es = RR.eval_set(request.param)
    scores = torch.from_numpy(arr["scores"])
    order = es.rank(scores).numpy()
    h = es._host
    rest = (es.binarization_point, es.rcut, es.ncut, es.map_cut, h["bnr"], h["idcg"], h["log2"])
    return js, arr, es, scores, order, rest, RR.matched_rows(es)


def test_ranking_rule_restatement_and_numpy_route_agree_with_the_goldens(case):
    js, arr, es, scores, order, rest, m = case
    assert np.array_equal(order, RR.rank_ref(arr["scores"], es._host["seg_begin"]))
    got = es.ranked_result(scores)
    assert got == js["ranking"] and list(got) == list(js["ranking"])


def test_nan_and_signed_zero_rule():
    """The stated choice: NaN behind everything (-inf included) in arrival order; -0.0 == +0.0 keep arrival order."""
    from matchmaker_amd.metrics import np_segment_rank
    sc = np.array([np.nan, -np.inf, 0.0, -0.0, np.nan, np.inf, -0.0, 1.0], np.float32)
    sb = np.array([0, 8])
    want = [5, 7, 2, 3, 6, 1, 0, 4]
    assert list(RR.rank_ref(sc, sb)) == want and list(np_segment_rank(sc, sb)) == want


def _forms(case):
    js = case[0]
    yield "plain", None, js["plain"]
    for t, want in js["single"].items():
        yield f"single{t}", int(t), want


def test_plain_and_single_threshold_against_the_goldens(case):
    js, arr, es, scores, order, rest, m = case
    h = es._host
    m_mean = int(m.max()) + es.n_queries
    for tag, threshold, want in _forms(case):
        ref = RR.metrics_ref(order, h["seg_begin"], h["grade"], None if threshold is None else h["cand_pos"], threshold, *rest)
        assert np.array_equal(ref[4], m)
        pq = tuple(x.numpy() for x in es.per_query(scores, threshold))
        assert np.array_equal(pq[0], ref[0]) and np.array_equal(pq[1], ref[1]), tag
        for side, name in ((ref[:4], "restatement"), (pq, "numpy route")):
            RR.assert_per_query(es, side, arr[tag + "_rr"], arr[tag + "_ap"], arr[tag + "_recall"], arr[tag + "_ndcg"], m,
                                f"{tag} {name}")
        RR.assert_dict(RR.dict_ref(*ref[:4], h["bnr"], es.evaluated_queries, es.rcut, es.ncut, es.map_cut), want, m_mean, tag)
        got = es.metrics_plain(scores) if threshold is None else es.metrics_single_candidate_threshold(scores, threshold)
        RR.assert_dict(got, want, m_mean, tag)
        d, rr, ap, rec, ndcg = (es.metrics_plain(scores, return_per_query=True) if threshold is None else
                                es.metrics_single_candidate_threshold(scores, threshold, return_per_query=True))
        assert _same(d, got) and np.array_equal(rr, arr[tag + "_rr"]) and np.array_equal(rec, arr[tag + "_recall"])
        assert ap.shape == arr[tag + "_ap"].shape and ndcg.shape == arr[tag + "_ndcg"].shape


def test_depth_sweep_against_the_goldens(case):
    js, arr, es, scores, order, rest, m = case
    h = es._host
    m_mean = int(m.max()) + es.n_queries
    for entry in js["depth"]:
        lo, hi = entry["range"]
        want = arr[f"depth_{lo}_{hi}"]
        ref = RR.depth_ref(order, h["seg_begin"], h["grade"], h["cand_pos"], hi, *rest)
        for chunk in (None, 1, 4):
            got = es.metrics_along_candidate_depth(scores, (lo, hi), query_chunk=chunk)
            assert list(got) == list(range(lo, hi + 1))
            for i, th in enumerate(range(lo, hi + 1)):
                w = dict(zip(entry["keys"], want[i]))
                RR.assert_dict(got[th], w, m_mean, f"depth {lo}-{hi} t={th} chunk={chunk}")
                if chunk is None:
                    RR.assert_dict(RR.dict_ref(ref[0][:, th - 1], ref[1][:, th - 1], ref[2][:, th - 1], ref[3][:, th - 1], h["bnr"],
                                               es.evaluated_queries, es.rcut, es.ncut, es.map_cut), w, m_mean, f"restatement t={th}")
                    one = es.metrics_single_candidate_threshold(scores, th)          # the sweep at t is the single form at t
                    RR.assert_dict(got[th], one, m_mean, f"sweep vs single t={th}")


def test_against_the_real_functions_when_the_reference_is_mounted():
    from oracle import ref_harness as R
    if not R.available():
        pytest.skip("reference tree not mounted")
    spec = importlib.util.spec_from_file_location("ref_core_metrics", os.path.join(R.REFERENCE_ROOT, "matchmaker", "utils", "core_metrics.py"))
    cm = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(cm)
    except Exception:
        pytest.skip("optional dependencies of the reference missing here")
    from matchmaker_amd.metrics import EvalSet, global_metric_config
    assert cm.global_metric_config == global_metric_config
    rng = np.random.default_rng(21)
    qids, dids, sc, qrels, cand = [], [], [], {}, {}
    for q in range(25):
        n = int(rng.integers(1, 50))
        docs = [f"d{int(x)}" for x in rng.permutation(70)[:n]]
        qids += [f"q{q}"] * n
        dids += docs
        sc += list(rng.integers(0, 6, n).astype(np.float32))
        if q % 6 != 2:
            qrels[f"q{q}"] = {f"d{int(x)}": int(rng.integers(0, 4)) for x in rng.permutation(70)[:int(rng.integers(1, 8))]}
        cand[f"q{q}"] = {d: int(p) + 1 for d, p in zip(docs, rng.permutation(n))}
    sc = torch.tensor(sc)
    unrolled = {}
    for q, d, s in zip(qids, dids, sc.tolist()):
        unrolled.setdefault(q, []).append((d, s))
    ranking = cm.unrolled_to_ranked_result(unrolled)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for bp in (1.0, 2.0):
            es = EvalSet(qids, dids, qrels, cand, binarization_point=bp)
            mm = int(RR.matched_rows(es).max()) + es.n_queries
            assert es.ranked_result(sc) == ranking
            RR.assert_dict(es.metrics_plain(sc), cm.calculate_metrics_plain(ranking, qrels, bp), mm)
            for t in (1, 4, 49):
                RR.assert_dict(es.metrics_single_candidate_threshold(sc, t),
                               cm.calculate_metrics_single_candidate_threshold(ranking, qrels, cand, t, bp), mm)
            want = cm.calculate_metrics_along_candidate_depth(ranking, qrels, cand, (3, 49), bp)
            got = es.metrics_along_candidate_depth(sc, (3, 49), query_chunk=6)
            assert list(got) == list(want)
            for t in want:
                RR.assert_dict(got[t], want[t], mm)


# ---- EvalSet's join ----------------------------------------------------------------------------------------------------------
def test_evalset_join_dict_order_duplicates_and_absent_queries():
    from matchmaker_amd.metrics import EvalSet, NOT_JUDGED
    qids = ["b", "a", "b", "c", "a", "b", "zz"]                     # interleaved arrival; "c" / "zz" are not in the qrels
    dids = ["d1", "d1", "d2", "d9", "d3", "d1", "d5"]               # d1 twice in b's list
    qrels = {"a": {"d3": 2, "d7": 1}, "b": {"d1": 1}, "never_ranked": {"d1": 3}}
    cand = {"a": {"d1": 2, "d3": 1}, "b": {"d1": 1, "d2": 2}}       # no candidate list for c / zz: they are not judged
    es = EvalSet(qids, dids, qrels, cand)
    assert es.qids == ["b", "a", "c", "zz"]                         # first-arrival order = the reference dict's key order
    assert es.docs == ["d1", "d2", "d1", "d1", "d3", "d9", "d5"]
    assert es.t["seg_begin"].tolist() == [0, 3, 5, 6, 7] and es.max_len == 3
    assert es.t["perm"].tolist() == [0, 2, 5, 1, 4, 3, 6]
    assert es.t["grade"].tolist() == [1, NOT_JUDGED, 1, NOT_JUDGED, 2, NOT_JUDGED, NOT_JUDGED]
    assert es.t["cand_pos"].tolist()[:5] == [1, 2, 1, 2, 1]
    assert es.t["bnr"].tolist() == [1, 2, 0, 0] and es.in_qrels.tolist() == [True, True, False, False]
    assert es.evaluated_queries == 2
    sc = torch.tensor([0.5, 1.0, 0.7, 0.1, 3.0, 0.5, 0.0])          # arrival order
    assert es.ranked_result(sc) == {"b": ["d2", "d1", "d1"], "a": ["d3", "d1"], "c": ["d9"], "zz": ["d5"]}
    d = es.metrics_plain(sc)
    assert d["QueriesRanked"] == 2 and d["QueriesWithRelevant@10"] == 2 and d["QueriesWithNoRelevant@10"] == 2
    assert d["MRR@10"] == (1 / 2 + 1) / 2 and d["Recall@10"] == (2 / 1 + 1 / 2) / 2      # the duplicate counts twice, as in the reference
    assert d["MedianRankGoldLabel@10"] == 1.5 and d["AverageRankGoldLabel@10"] == 1.5
    for bad_qrels, bad_cand in (({"a": {"d3": -1}}, None), ({"a": {"d3": 0.5}}, None), (qrels, {"b": {"d1": 1, "d2": 2}}),
                                (qrels, {"a": {"d1": 2, "d3": 1}, "b": {"d1": 1}})):
        with pytest.raises(ValueError):
            EvalSet(qids, dids, bad_qrels, bad_cand)
    with pytest.raises(ValueError):
        EvalSet(qids, dids[:-1], qrels)


def test_value_errors_segment_longer_than_hi_and_zero_evaluated_queries():
    from matchmaker_amd.metrics import EvalSet
    es = EvalSet(["q"] * 5, list("abcde"), {"q": {"a": 1}}, {"q": {d: i + 1 for i, d in enumerate("abcde")}})
    sc = torch.arange(5.0)
    with pytest.raises(ValueError, match="more than candidate_range"):
        es.metrics_along_candidate_depth(sc, (1, 4))
    assert list(es.metrics_along_candidate_depth(sc, (5, 5))) == [5]
    with pytest.raises(ValueError):
        es.metrics_along_candidate_depth(sc, (3, 2))
    none = EvalSet(["q"] * 2, ["a", "b"], {"other": {"a": 1}}, {"q": {"a": 1, "b": 2}})
    for call in (lambda: none.metrics_plain(sc[:2]), lambda: none.metrics_single_candidate_threshold(sc[:2], 1),
                 lambda: none.metrics_along_candidate_depth(sc[:2], (1, 2))):
        with pytest.raises(ValueError, match="none of the ranked queries"):
            call()
    assert none.ranked_result(sc[:2]) == {"q": ["b", "a"]}
    with pytest.raises(ValueError):
        EvalSet(["q"], ["a"], {"q": {"a": 1}}).metrics_single_candidate_threshold(sc[:1], 1)      # no candidate ranking


# ---- header, binding, refusals -----------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays_4():
    from matchmaker_amd import build, _lib
    from tests import abi
    L = abi.assert_bound(SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    for name in SYMBOLS:
        assert re.search(name + r" \(additive: MM_ABI_VERSION unchanged\)\s+\* Replaces: .*core_metrics\.py:\d+", hdr), name
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION and "#define MM_ABI_VERSION 4" in hdr
    assert "rank_metrics.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "rank_metrics.hip"))
    assert f"#define MM_RANK_MAX_LEN {_lib.RANK_MAX_LEN}" in hdr and 4096 <= _lib.RANK_MAX_LEN and _lib.RANK_MAX_LEN * 8 <= 160 * 1024
    src = open(os.path.join(build.CSRC, "rank_metrics.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")            # two calls are bit-equal by construction
    assert "bitonic_device.h" in src and "bitonic_device.h" in open(os.path.join(build.CSRC, "colbert_candidates.hip")).read()


def test_header_compiles_as_c_and_a_c_client_is_refused_before_any_launch(tmp_path):
    from tests import abi
    abi.run_c_client(tmp_path, r"""
#include <stdio.h>
#include <string.h>
#include "mm_native.h"
int main(void) {
  int32_t cut[2] = {3, 10};
  int32_t bad[1] = {0};
  int dummy = 0;
  void* p = &dummy;   /* never dereferenced: every call below is refused by the host-side checks */
  if (MM_ABI_VERSION != 4 || MM_RANK_MAX_LEN < 4096 || MM_RANK_NOT_JUDGED >= 0) return 1;
  if (mm_segment_rank_fwd(p, MM_F32, p, 10, 1, MM_RANK_MAX_LEN + 1, p, NULL) != MM_EUNSUPPORTED) return 2;
  if (!strstr(mm_last_error(), "max_len")) return 3;
  if (mm_segment_rank_fwd(NULL, MM_F32, NULL, 10, 1, 10, NULL, NULL) != MM_EINVAL) return 4;
  if (mm_segment_rank_fwd(p, 7, p, 10, 1, 10, p, NULL) != MM_EUNSUPPORTED) return 5;
  if (mm_segment_rank_fwd(p, MM_F32, p, -1, 1, 10, p, NULL) != MM_EINVAL) return 6;
  if (mm_segment_rank_fwd(p, MM_F32, p, 2147483648LL, 1, 10, p, NULL) != MM_EUNSUPPORTED) return 7;
  if (mm_segment_rank_fwd(NULL, MM_F32, NULL, 0, 3, 10, NULL, NULL) != MM_OK) return 8;      /* N = 0 */
  if (mm_segment_rank_fwd(NULL, MM_BF16, NULL, 5, 0, 10, NULL, NULL) != MM_OK) return 9;     /* nq = 0 */
  if (mm_rank_metrics_fwd(p, p, p, NULL, 10, 1, 5, 1.0, cut, 9, cut, 2, 10, p, p, p, 12, p, p, p, p, NULL) != MM_EUNSUPPORTED) return 10;
  if (mm_rank_metrics_fwd(p, p, p, NULL, 10, 1, 5, 1.0, cut, 2, cut, 2, 10, p, p, p, 10, p, p, p, p, NULL) != MM_EINVAL) return 11;  /* log2 table too short */
  if (mm_rank_metrics_fwd(p, p, p, NULL, 10, 1, 5, 1.0, bad, 1, cut, 2, 10, p, p, p, 12, p, p, p, p, NULL) != MM_EINVAL) return 12;
  if (mm_rank_metrics_fwd(p, p, p, NULL, 10, 1, 5, 1.0, cut, 2, cut, 2, 0, p, p, p, 12, p, p, p, p, NULL) != MM_EINVAL) return 13;
  if (mm_rank_metrics_fwd(p, NULL, p, NULL, 10, 1, 5, 1.0, cut, 2, cut, 2, 10, p, p, p, 12, p, p, p, p, NULL) != MM_EINVAL) return 14;
  if (mm_rank_metrics_fwd(NULL, NULL, NULL, NULL, 0, 0, 5, 1.0, cut, 2, cut, 2, 10, NULL, NULL, NULL, 12, NULL, NULL, NULL, NULL, NULL) != MM_OK) return 15;
  if (mm_rank_metrics_depth_fwd(p, p, p, p, 10, 1, MM_RANK_MAX_LEN + 1, 1.0, cut, 2, cut, 2, 10, p, p, p, 12, p, p, p, p, NULL) != MM_EUNSUPPORTED) return 16;
  if (mm_rank_metrics_depth_fwd(p, p, p, p, 10, 1, 0, 1.0, cut, 2, cut, 2, 10, p, p, p, 12, p, p, p, p, NULL) != MM_EINVAL) return 17;
  if (mm_rank_metrics_depth_fwd(p, p, p, NULL, 10, 1, 8, 1.0, cut, 2, cut, 2, 10, p, p, p, 12, p, p, p, p, NULL) != MM_EINVAL) return 18;
  if (strlen(mm_last_error()) == 0) return 19;
  printf("c client ok: %s\n", mm_last_error());
  return 0;
}
""")


def test_python_refusals_come_before_any_launch():
    """CPU tensors, wrong dtypes and shapes, bounds above the native limit: NativeError in the house wording, with no device."""
    from matchmaker_amd import ops, _lib
    from matchmaker_amd.ops import NativeError
    s, sb = torch.zeros(4), torch.tensor([0, 4])
    with pytest.raises(NativeError, match="need HIP device tensors"):
        ops.segment_rank(s, sb, 4)
    with pytest.raises(NativeError, match="need HIP device tensors"):
        ops.rank_metrics(s.int(), sb, s.int(), None, 3, 1.0, [10], [10], 10, torch.zeros(1, dtype=torch.int32),
                         torch.zeros(1, 1, dtype=torch.float64), torch.zeros(12, dtype=torch.float64))
    class Cuda(torch.Tensor):      # a tensor that claims to be on the device: the shape / dtype / limit checks run before any use
        is_cuda = True

    def fake(*shape, dtype):
        return torch.empty(shape, dtype=dtype).as_subclass(Cuda)

    with pytest.raises(NativeError, match="scores must be"):
        ops.segment_rank(fake(4, dtype=torch.int32), fake(2, dtype=torch.int64), 4)
    with pytest.raises(NativeError, match="seg_begin must be int64"):
        ops.segment_rank(fake(4, dtype=torch.float32), fake(2, dtype=torch.int32), 4)
    with pytest.raises(NativeError, match="max_len=8193 outside") as e:
        ops.segment_rank(fake(4, dtype=torch.float32), fake(2, dtype=torch.int64), ops.RANK_MAX_LEN + 1)
    assert e.value.code == _lib.MM_EUNSUPPORTED
    i32, f64 = torch.int32, torch.float64
    good = dict(order=fake(4, dtype=i32), seg_begin=fake(2, dtype=torch.int64), grade=fake(4, dtype=i32), cand_pos=fake(4, dtype=i32),
                binarization_point=1.0, mrr_cutoffs=[10], ndcg_cutoffs=[3, 10], map_cutoff=10,
                binary_num_relevant=fake(1, dtype=i32), idcg=fake(1, 2, dtype=f64), log2_table=fake(12, dtype=f64))
    for change, msg in ((dict(grade=fake(3, dtype=i32)), "grade must be int32"), (dict(order=fake(4, dtype=torch.int64)), "order must be"),
                        (dict(mrr_cutoffs=list(range(1, 10))), "at most 8 cutoffs"), (dict(ndcg_cutoffs=[0, 3]), "each >= 1"),
                        (dict(idcg=fake(1, 3, dtype=f64)), "idcg must be float64"), (dict(log2_table=fake(10, dtype=f64)), "log2_table must be"),
                        (dict(binary_num_relevant=fake(2, dtype=i32)), "binary_num_relevant must be"), (dict(map_cutoff=0), "map_cutoff=0")):
        with pytest.raises(NativeError, match=msg):
            ops.rank_metrics(threshold=5, **{**good, **change})
        with pytest.raises(NativeError, match=msg):
            ops.rank_metrics_depth(hi=8, **{**good, **change})
    with pytest.raises(NativeError, match="hi=8193 outside"):
        ops.rank_metrics_depth(hi=ops.RANK_MAX_LEN + 1, **good)
    with pytest.raises(NativeError, match="cand_pos is needed"):
        ops.rank_metrics_depth(hi=8, **{**good, "cand_pos": None})


def test_fake_rule_of_the_registered_op():
    import matchmaker_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        s = torch.empty(100, dtype=torch.bfloat16, device="cuda")
        sb = torch.empty(5, dtype=torch.int64, device="cuda")
        out = torch.ops.mm_native.segment_rank(s, sb, 40)
        assert out.shape == (100,) and out.dtype == torch.int32 and out.device.type == "cuda"
    with pytest.raises(NotImplementedError):
        torch.ops.mm_native.segment_rank(torch.zeros(4), torch.tensor([0, 4]), 4)      # no CPU kernel
