"""CPU: the exact-arithmetic MaxSim case table (tests/maxsim_exact_cases.py) keeps its promises.  The bit comparison of
tests/test_maxsim_exact_gpu.py rests on them: values exact in the case's dtype, every similarity and output a small multiple of
1/64 (gradients: 1/16), every planted row the strict unique maximum of its token, every planted edge load-bearing (the float64
expectation changes when that one edge is mutated), and every kernel the dispatch can pick reached by a case."""
import numpy as np
import pytest
import torch

from tests import maxsim_exact_cases as C

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
ROWS = pytest.mark.parametrize("row", C.TABLE, ids=C.row_name)


def _multiple(x, step, what):
    x = np.asarray(x, dtype=np.float64) / step
    assert (x == np.round(x)).all(), f"{what}: not a multiple of {step}"
    assert np.abs(x).max(initial=0.0) < 2.0 ** 24, f"{what}: {np.abs(x).max() * step} is not below 2^24 x {step}"


def test_case_names_are_unique_and_the_table_is_deterministic():
    names = [C.row_name(r) for r in C.TABLE]
    assert len(set(names)) == len(names)
    row = C.TABLE[0]
    a = C.build(*row)
    C.build.cache_clear()
    b = C.build(*row)
    assert a is not b and (a.q == b.q).all() and (a.d == b.d).all() and (a.dm == b.dm).all() and a.edges == b.edges
    assert {c.enc for c in C.cases()} == set(C.ENCODINGS)
    for entry in ("maxsim", "inbatch", "ragged", "bwd"):          # each mask encoding for each entry point
        assert {c.enc for c in C.cases(entry)} == set(C.ENCODINGS), entry


@ROWS
def test_inputs_are_exact_in_the_dtype_and_every_sum_is_exact_in_fp32(row):
    c = C.build(*row)
    for name, x in (("q", c.q), ("d", c.d), ("tokens", c.tokens), ("grad_out", c.go)):
        if x is None:
            continue
        dt = torch.float32 if name == "grad_out" else DT[c.dtype]
        assert (torch.from_numpy(x).to(dt).double().numpy() == x).all(), f"{name} does not survive {dt}"
        assert (np.abs(x * 8) <= (16 if name == "grad_out" else 4)).all() and (x * 8 == np.round(x * 8)).all()
    assert c.E <= 768                                  # |<q, d>| <= E / 4 <= 192
    if c.entry == "inbatch":
        sims = np.einsum("ite,jpe->ijtp", c.q, c.d)
    else:
        sims = np.einsum("pte,pde->ptd", c.q[np.arange(c.d.shape[0]) // c.ppq], c.d)
    _multiple(sims, 1 / 64, "similarities")
    assert np.abs(sims).max() <= c.E / 4
    out = C.expect(c)
    if c.entry == "bwd":
        _multiple(out[0], 1 / 16, "grad_q")
        _multiple(out[1], 1 / 16, "grad_d")
        assert set(np.abs(c.go)) <= {0.5, 1.0, 2.0}
    else:
        _multiple(out, 1 / 64, "scores")
        assert out.shape == ((c.q.shape[0], c.d.shape[0]) if c.entry == "inbatch" else (c.d.shape[0],))


def _assert_planted(c, e):
    """The planted position is the strict unique maximum of its token among the unmasked rows (ties: only the planted ones)."""
    top = c.E / 4
    if e.kind == "qpad":
        assert c.qm[e.query, e.tok] == 0
        return
    assert c.qm[e.query, e.tok] == 1 and e.tok == c.ptok[e.k] and (c.q[:, e.tok] == c.pats[e.k]).all()
    s = c.d[e.doc] @ c.q[e.query, e.tok]
    keep = c.dm[e.doc] != 0
    at_top = set(np.nonzero(keep & (s == top))[0])
    assert (s[keep] <= top).all()
    if e.kind in ("row", "qtok"):
        assert at_top == {e.rows[0]}, (e, at_top)
    elif e.kind == "dup":
        assert at_top == set(e.rows) and e.rows[1] - e.rows[0] >= 2, (e, at_top)
    elif e.kind == "hole_copy":
        assert at_top == {e.rows[1]} and not keep[e.rows[0]] and s[e.rows[0]] == top and e.rows[0] < e.rows[1], (e, at_top)
    else:
        assert e.kind in ("pad", "hole", "pre")
        assert not at_top and not keep[e.rows[0]] and s[e.rows[0]] == top, (e, at_top)


@ROWS
def test_every_planted_edge_is_a_strict_maximum_and_load_bearing(row):
    c = C.build(*row)
    base = C.expect(c)
    assert c.edges
    for e in c.edges:
        _assert_planted(c, e)
        qm, dm, sel = C.mutated_masks(c, e)
        assert (qm != c.qm).sum() + (dm != c.dm).sum() == (2 if e.kind == "dup" and c.entry != "bwd" else 1)
        was, now = C.take(c, base, sel), C.expect(c, qm, dm, sel)
        if c.entry == "bwd":
            changed = (was[0] != now[0]).any() or (was[1] != now[1]).any()
        else:
            changed = (was != now).any()
        assert changed, f"{c.name}: {e} is not load-bearing: the expectation is the same without it"


def _doc_lens(c):
    """Per document: its prefix length, or -1 for a non-prefix mask."""
    n = c.dm.sum(1)
    prefix = (c.dm == (np.arange(c.dm.shape[1])[None] < n[:, None])).all(1)
    return np.where(prefix, n, -1)


@ROWS
def test_the_planted_positions_cover_what_exists_at_the_shape(row):
    c = C.build(*row)
    Q = c.Q
    assert set(c.ptok) >= {t for t in (0, Q - 1, 31, 32) if t < Q} and len(c.ptok) == min(Q, C.N_PAT)
    kinds = {e.kind for e in c.edges}
    rows_of = lambda kind: {(e.doc, e.rows[0]) for e in c.edges if e.kind == kind}
    lens = _doc_lens(c)
    if c.entry == "ragged":
        off = 1                                       # row 0 of the restatement is the store row in front of the range
        L = max(c.lens)
        want = {r + off for r in (0, 31, 32, 32 * ((L - 1) // 32), L - 1)}
        assert want <= {r for d, r in rows_of("row") if c.dm[d].sum() == L}
        assert {"row", "pre", "pad", "qtok", "qpad"} <= kinds
        assert 0 in c.lens and len(set(c.cand)) < len(c.cand) and len(c.lens) - 1 in c.cand      # empty, repeated, last
        assert any(b % 32 and e % 32 and b // 32 == (e - 1) // 32 for b, e in zip(c.begin, c.end) if e > b)
        assert c.end.max() == c.tokens.shape[0]
        return
    D, B = c.D, c.d.shape[0]
    full = {r for d, r in rows_of("row") if lens[d] == D}
    assert full >= {r for r in (0, D - 1, 31, 32, 32 * ((D - 1) // 32)) if r < D}, "rows of the document with len == D"
    assert (lens == D).any() and (lens == 0).any() and (c.qm.sum(1) < Q).any() == (Q >= 2 and c.q.shape[0] >= 2)
    assert any(lens[d] == 0 and r == 0 for d, r in rows_of("pad")), "the fully padded document holds a pattern"
    if D >= 2:
        assert any(0 < lens[d] == r for d, r in rows_of("pad")), "row `len` holds a pattern"
        assert any(0 < lens[d] == r + 1 < D for d, r in rows_of("row")), "row len - 1 of a padded document"
    if D >= 7 and B >= 4:
        assert "dup" in kinds
        if c.enc != "len":
            assert ("hole_copy" if c.entry == "bwd" else "hole") in kinds and (lens == -1).any()
            nonprefix_q = (c.qm != (np.arange(Q)[None] < c.qm.sum(1)[:, None])).any()
            assert nonprefix_q == (Q > len(c.ptok) and c.q.shape[0] >= 3), "a hole in a query mask"
    if Q >= 2 and c.q.shape[0] >= 2:
        assert "qpad" in kinds and "qtok" in kinds


def test_the_table_reaches_every_kernel_the_dispatch_can_pick():
    reached = {}
    for c in C.cases():
        reached.setdefault(C.expected_kernel(c), set()).add(c.dtype)
    for branch, dtypes in C.REQUIRED.items():
        assert branch in reached, f"no case reaches {branch}"
        assert set(dtypes) <= reached[branch], f"{branch}: reached with {sorted(reached[branch])} only, needs {dtypes}"
    assert set(reached) <= set(C.REQUIRED), f"branches without a requirement: {set(reached) - set(C.REQUIRED)}"
    kernels = {b.split(":")[0] for b in C.REQUIRED}
    for switch, hits in C.SWITCHES.items():
        assert hits is None or set(hits) <= kernels, switch


def test_the_dispatch_restatement_knows_the_thresholds():
    """The numbers the table's shapes were chosen by (launch_geometry.h wave_split, 256 CUs x 4 wavefronts)."""
    assert C.wave_split(1024, 1024) == (1, 1024) and C.wave_split(1025, 1024) == (2, 513) and 1025 - 2 * 512 == 1
    assert C.wave_split(600, 1024) == (1, 600) and 600 * 2 > 1024 and 4 * 2 <= 1024
    assert C.wave_split(0, 1024) == (1, 0)
    assert 320 * 4 + 1024 + 1540 * 10 * 4 > 60 * 1024 >= 70 * 4 + 1024 + 95 * 3 * 4
