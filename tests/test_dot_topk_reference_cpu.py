"""Pins tests/dot_topk_reference.py: both restatements against plain Python loops on tiny inputs with planted ties and
padding, and the PRECONDITIONS of the cases tests/test_dot_topk_exact_gpu.py runs on the device — exact representability of
the stores, how many documents sit at or above the k-th score against the candidate capacity, which rows take the
full-sort path — from the reference alone, before any device call."""
import numpy as np
import pytest

from tests import dot_topk_reference as R


def _loop_topk(q, c, k):
    out_s, out_i = [], []
    for qv in q:
        sc = [float(sum(float(a) * float(b) for a, b in zip(qv, row))) for row in c]
        rows = list(range(len(c)))
        picked = []
        while rows and len(picked) < k:          # the largest score; the first (lowest) row among equals
            best = rows[0]
            for r in rows[1:]:
                if sc[r] > sc[best]:
                    best = r
            picked.append(best)
            rows.remove(best)
        out_s.append([sc[r] for r in picked] + [-np.inf] * (k - len(picked)))
        out_i.append(picked + [-1] * (k - len(picked)))
    return np.array(out_s), np.array(out_i, np.int64)


def _loop_merge(scores, ids, k):
    out_s, out_i = [], []
    for srow, irow in zip(scores.tolist(), ids.tolist()):
        pos = [p for p in range(len(irow)) if irow[p] >= 0]
        picked = []
        while pos and len(picked) < k:           # the largest score; the first position among equals
            best = pos[0]
            for p in pos[1:]:
                if srow[p] > srow[best]:
                    best = p
            picked.append(best)
            pos.remove(best)
        out_s.append([srow[p] for p in picked] + [-np.inf] * (k - len(picked)))
        out_i.append([irow[p] for p in picked] + [-1] * (k - len(picked)))
    return np.array(out_s), np.array(out_i, np.int64)


@pytest.mark.parametrize("k", [1, 3, 7, 12])
def test_dot_topk_exact_is_the_plain_loop_with_planted_ties(k):
    q = R.ternary_store(3, 8, 1)
    c = R.ternary_store(9, 8, 2)
    c[5] = c[1]
    c[7] = c[1]              # rows 1, 5, 7 tie for every query
    c[2] = 0
    c[8] = 0                 # rows 2, 8 score 0
    q[2] = 0                 # every row ties
    s, i = R.dot_topk_exact(q, c, k)
    ls, li = _loop_topk(q, c, k)
    np.testing.assert_array_equal(s, ls)
    np.testing.assert_array_equal(i, li)
    np.testing.assert_array_equal(i[2, : min(k, 9)], np.arange(min(k, 9)))
    if k > 9:
        assert (i[:, 9:] == -1).all() and np.isneginf(s[:, 9:]).all()


@pytest.mark.parametrize("k", [1, 4, 6, 9])
def test_topk_merge_exact_is_the_plain_loop_with_padding_and_ties(k):
    s = np.array([[2, 1e30, 2, 5, 2, -np.inf, 5, 1e30],
                  [1e30, np.inf, 3, 3, 3, 3, 3, 3],
                  [4, 4, -np.inf, 4, 1e30, 0, 0, 0]], np.float32)
    ids = np.array([[7, -1, 3, 9, 1, 4, 2, -5],
                    [-1, -1, -1, -1, -1, -1, -1, -1],
                    [1 << 40, 5, 6, (1 << 40) + 1, -1, 2, 1, 0]], np.int64)
    ms, mi = R.topk_merge_exact(s, ids, k)
    ls, li = _loop_merge(s, ids, k)
    np.testing.assert_array_equal(ms, ls)
    np.testing.assert_array_equal(mi, li)
    assert (mi[1] == -1).all() and np.isneginf(ms[1]).all()
    if k == 9:
        np.testing.assert_array_equal(mi[0], [9, 2, 7, 3, 1, 4, -1, -1, -1])     # the -inf entry precedes the padding
        np.testing.assert_array_equal(mi[2], [1 << 40, 5, (1 << 40) + 1, 2, 1, 0, 6, -1, -1])


def test_tie_stats_counts_the_group_at_the_kth_score():
    full = np.array([[5, 3, 3, 3, 1, 0], [2, 2, 2, 2, 2, 2], [9, 8, 7, 6, 5, 4]], np.float64)
    at_or_above, group = R.tie_stats(full, 2)
    np.testing.assert_array_equal(at_or_above, [4, 6, 2])
    np.testing.assert_array_equal(group, [3, 6, 1])
    at_or_above, group = R.tie_stats(full, 10)        # k > N: the N-th score
    np.testing.assert_array_equal(at_or_above, [6, 6, 6])
    np.testing.assert_array_equal(group, [1, 6, 1])


def test_cap_mirrors_the_documented_capacity():
    assert R.cap_of(20000, 1000) == 4096 and R.cap_of(20000, 10) == 1024 and R.cap_of(3000, 100) == 4096
    assert R.cap_of(40000, 1025) == 8192 and R.cap_of(40000, 2000) == 8192 and R.cap_of(40000, 4096) == 16384
    assert R.cap_of(3000, 4096) == 16384 and R.cap_of(70001, 400) == 2048 and R.cap_of(4097, 100) == 1024


@pytest.mark.parametrize("kind", ["ternary", "quarter", "nonpos"])
def test_stores_are_exact_in_both_16_bit_formats_and_in_fp32_sums(kind):
    import torch
    q, c = R.inputs(kind, 6, 300, 768, 5)
    for a in (q, c):
        t = torch.from_numpy(a)
        assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    # every product is a multiple of 1/16 and sum |q_i c_i| < 2^24 / 16: every partial sum is an fp32 value in any order
    bound = np.abs(q).astype(np.float64) @ np.abs(c).astype(np.float64).T
    assert bound.max() * 16 < 2 ** 24
    assert np.array_equal(q * 4, np.round(q * 4)) and np.array_equal(c * 4, np.round(c * 4))
    if kind == "nonpos":
        assert R.scores64(q, c).max() < 0


ALL_CONVERGING = R.SWEEP + R.LARGE_K + R.NEGATIVE + [R.MANY_GROUPS, R.RAW_ABI]


@pytest.mark.parametrize("case", ALL_CONVERGING, ids=[c[0] for c in ALL_CONVERGING])
def test_converging_cases_fit_the_candidate_capacity(case):
    _, kind, _, nq, N, E, k, _ = case
    assert E in (128, 256, 384, 512, 768) and 1 <= k <= R.K_MAX
    q, c = R.case_inputs(case)
    full = R.scores64(q, c)
    at_or_above, _ = R.tie_stats(full, k)
    assert at_or_above.max() <= R.cap_of(N, k), (at_or_above.max(), R.cap_of(N, k))
    if kind == "nonpos":
        assert full.max() < 0            # the whole top-k is negative


def test_sweep_covers_every_dim_in_each_dtype_and_the_two_set_form():
    for dt in ("float16", "bfloat16"):
        assert {c[5] for c in R.SWEEP if c[2] == dt} == {128, 256, 384, 512, 768}
        assert any(c[5] == 768 and c[3] > 128 for c in R.SWEEP if c[2] == dt)
    assert {c[3] for c in R.SWEEP} == {1, 128, 129, 257}
    assert {c[4] for c in R.SWEEP} == {1, 31, 33, 4096, 4097, 20000, 70001}
    assert {c[6] for c in R.SWEEP} == {1, 10, 100, 1000}
    assert {c[1] for c in R.SWEEP} == {"ternary", "quarter"}
    assert R.MANY_GROUPS[3] > 32 * 256 and R.MANY_GROUPS[4] > 4096


def test_mixed_tie_case_has_rows_on_both_sides_of_the_selection_limit():
    q, c = R.mixed_ties_inputs()
    at_or_above, _ = R.tie_stats(R.scores64(q, c), R.MIXED_TIES[6])
    assert at_or_above.max() > R.SEL_MAX and at_or_above.min() <= R.SEL_MAX, at_or_above
    assert at_or_above.min() >= 1000 and at_or_above.max() <= R.cap_of(20000, 1000), at_or_above


def test_planted_groups_are_the_strict_best_and_sit_where_the_cases_need_them():
    for make, n_group, converges in ((R.planted_1500, 1500, True), (R.planted_5000, 5000, False),
                                     (R.planted_sampled_1100, 1100, True)):
        q, c, rows, k = make()
        N, E = c.shape
        full = R.scores64(q, c)
        assert rows.size == n_group == np.unique(rows).size
        assert (full[0, rows] == E).all() and (np.delete(full[0], rows) < E).all()
        at_or_above, group = R.tie_stats(full, k)
        assert at_or_above[0] == group[0] == n_group > R.SEL_MAX
        if converges:
            assert at_or_above.max() <= R.cap_of(N, k)
            s, i = R.topk_of_scores(full[:1], k)
            np.testing.assert_array_equal(i[0], rows[:k])          # the k lowest rows of the group, ascending
            assert (s[0] == E).all()
        else:
            assert at_or_above[0] > R.cap_of(N, k)
    # the sampled group: all of it among the first 1,100 sample positions, so that every one of the 1,024 per-thread maxima
    # of the threshold select is the group's score and more than 1,024 sample keys reach it; m <= 256 puts the select there
    q, c, rows, k = R.planted_sampled_1100()
    N = c.shape[0]
    stride = N // R.SAMPLE
    assert (rows % stride == 0).all() and (rows // stride).max() < 1100 and rows.size > 1024
    assert int(2.5 * k * R.SAMPLE / N + 0.5) <= 256


def test_all_zero_query_cases():
    assert R.cap_of(3000, 100) >= 3000            # N = 3000: every document ties and all of them fit -> rows 0 .. 99
    assert R.cap_of(20000, 100) < 20000           # N = 20000: they cannot fit -> the documented error


def test_raw_abi_case_thresholds_land_where_the_statuses_need_them():
    _, _, _, nq, N, E, k, _ = R.RAW_ABI
    q, c = R.case_inputs(R.RAW_ABI)
    full = R.scores64(q, c)
    cap = R.cap_of(N, k)
    assert (R.sampled_survivors(full, k, 1e-3) < k).all()                 # status 1 on every row
    assert (R.sampled_survivors(full, k, 100.0) > cap).all()              # status 2 on every row
    mid = R.sampled_survivors(full, k, 1.0)
    assert (mid >= k).all() and (mid <= cap).all(), mid                   # status 0 on every row


def test_merge_inputs_hold_what_the_merge_cases_claim():
    for n_in in (1, 2, 1000, 16384):
        s, ids = R.merge_inputs(n_in)
        assert s.shape == ids.shape == (3, n_in) and s.dtype == np.float32 and ids.dtype == np.int64
        assert (ids[1] == -1).all() and ids[ids >= 0].min() >= 1 << 40
        assert np.isneginf(s[2, n_in // 2]) and ids[2, n_in // 2] >= 0
        if n_in >= 1000:
            assert (ids[0] < 0).sum() > 100 and (s[0][ids[0] < 0] == np.float32(1e30)).all()
            assert np.unique(s[0][ids[0] >= 0]).size == 8
        ms, mi = R.topk_merge_exact(s, ids, n_in + 5)
        assert (mi[1] == -1).all() and (mi[:, -5:] == -1).all() and np.isfinite(ms[0, 0])
        last = (mi[2] >= 0).sum() - 1
        assert mi[2, last] == ids[2, n_in // 2] and np.isneginf(ms[2, last])   # the valid -inf entry: last before the padding


def test_shards_end_in_one_smaller_than_k():
    assert R.SHARDS == (9000, 7000, 3950, 50) and sum(R.SHARDS) == 20000
    q, c = R.shard_inputs()
    at_or_above, _ = R.tie_stats(R.scores64(q, c), 100)
    assert at_or_above.max() <= R.cap_of(20000, 100)
    lo = 0
    for n in R.SHARDS:
        a, _ = R.tie_stats(R.scores64(q, c[lo: lo + n]), 100)
        assert a.max() <= R.cap_of(n, 100)
        lo += n
