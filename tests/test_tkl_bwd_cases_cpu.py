"""The planted cases of tests/tkl_bwd_cases.py, proved without a GPU: the window scores realise the region layout each case
names, every float64 gradient is non-trivial, the map of structural zeros agrees with the float64 gradient, and a float32
evaluation of the same 15 windows (the torch restatement on the CPU) stays inside the bound the GPU tests hold mm_tkl_bwd to —
so a case that fails on the device is a wrong kernel, not an unattainable bound."""
import pytest
import torch

from tests import tkl_bwd_cases as T
from tests.tkl_window_reference import selected_window_scores

SATS = ["embedding", "log"]


@pytest.mark.parametrize("name", list(T.CASES))
def test_planted_window_scores_realise_the_layout_the_case_names(name):
    c = T.planted(name, "embedding")
    top, idx = T.selected_windows(c["win"])
    W = c["win"].shape[1]
    assert W == 186 and c["C"] == 10
    for b, (doc, want) in enumerate(zip(T.CASES[name], c["picks"])):
        got = tuple(int(x) for x in top[b])
        assert got == tuple(want), (name, b, got)
        dist = lambda p: (abs(p[0] - p[1]), abs(p[1] - p[2]), abs(p[0] - p[2]))
        assert dist(got) == dist(want)
        assert min(dist(got)) >= 15                                      # the suppression radius of the region search
    d = {b: tuple(abs(p[i] - p[j]) for i, j in ((0, 1), (1, 2), (0, 2))) for b, p in enumerate(c["picks"])}
    if name == "separate":
        assert all(min(v) >= 19 for v in d.values())
    elif name == "overlap_15_apart":
        assert d[0] == (15, 15, 30) and d[1] == (15, 15, 30)
    elif name == "adjacent_16_apart":
        assert d[0] == (16, 16, 32) and d[1] == (16, 16, 32)
    elif name == "overlap_edge_18_19":
        assert d[0] == (18, 18, 36) and d[1] == (19, 19, 38) and d[2] == (15, 35, 20)
    elif name == "ends_clamp":
        assert c["picks"][0][0] == 0 and c["picks"][0][2] == W - 1 and c["picks"][1][0] == W - 2
        assert (idx[0] == 0).sum() == 3 and (idx[0] == W - 1).sum() == 3     # the peak and its clamped neighbours -1, -2 | +1, +2
    elif name == "tied_peaks":
        win = c["win"]
        assert win[0, 40] == win[0, 120] and win[1, 40] == win[1, 50] and win[2, 66] == win[2, 130]
        assert 50 not in c["picks"][1]
    elif name in ("shorter_than_a_window", "one_token"):
        n_tok = T.CASES[name][0]["d_len"]
        assert int((c["win"][0] != 0).sum()) == (n_tok + 1) // 2
        assert c["picks"][0] == (0, 15, 30) and c["win"][0, 15] == 0 and c["win"][0, 30] == 0
        assert (c["win"][0, 13] != 0) == (name == "shorter_than_a_window")   # a neighbour of an empty pick that holds tokens
    elif name == "hole_empties_a_chunk":
        assert c["chunks"].shape[0] == 2 * 10 - 3                           # three chunks dropped
        assert (c["win"][0, 80:86] == 0).all() and c["win"][0, 79] != 0 and c["win"][0, 86] != 0
        assert c["win"][1, 39] != 0 and (c["win"][1, 40:66] == 0).all() and c["win"][1, 80] != 0


@pytest.mark.parametrize("sat", SATS)
@pytest.mark.parametrize("name", list(T.CASES))
def test_float64_gradients_are_not_vacuous_and_vanish_exactly_on_the_structural_zeros(name, sat):
    c = T.planted(name, sat)
    gq, gc, gp = T.planted_reference(name, sat)
    assert set(gp) == set(T.param_names(sat))
    for n, g in [("grad_q", gq), ("grad_chunks", gc)] + list(gp.items()):
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, (name, sat, n)
    for b in range(c["B"]):
        assert float(gq[b].abs().max()) > 0, (name, sat, b)
    zero = T.structural_zero_rows(c["win"], c["slot"], c["C"])
    assert zero.shape == gc.shape[:2] and zero[:, :5].all() and zero[:, 45:].all()
    assert (gc[zero] == 0).all()
    assert float(gc[~zero].abs().max()) > 0
    # every row that is read and holds a token carries gradient; a padding row that is read gets its zero by arithmetic
    touched = gc.abs().amax(-1) > 0
    assert torch.equal(touched, ~zero & (c["cmask"] != 0) & _has_live_window(c))


def _has_live_window(c):
    """bool [P, 50]: rows read by a selected window that holds a token (an empty window is the constant 0, :282)."""
    win, C = c["win"], c["C"]
    B = win.shape[0]
    _, idx = T.selected_windows(win)
    slot2p = torch.full((B * C,), -1, dtype=torch.long)
    slot2p[c["slot"].long()] = torch.arange(c["slot"].numel())
    read = torch.zeros(c["chunks"].shape[0], 50, dtype=torch.bool)
    for b in range(B):
        for w in set(idx[b].tolist()):
            if win[b, w] == 0:
                continue
            for t in range(2 * w, min(2 * w + 30, C * 40)):
                if slot2p[b * C + t // 40] >= 0:
                    read[slot2p[b * C + t // 40], t % 40 + 5] = True
    return read


@pytest.mark.parametrize("sat", SATS)
@pytest.mark.parametrize("name", list(T.CASES))
def test_a_float32_evaluation_meets_the_bound_against_float64(name, sat):
    """The float32 restatement on the CPU against float64 at rtol 2e-3, atol 3e-4 max(1, |want|max): the ratio error / bound,
    printed per tensor, is recorded beside the table in tests/tkl_bwd_cases.py."""
    c = T.planted(name, sat)
    gq64, gc64, gp64 = T.planted_reference(name, sat)
    m = c["model"]
    for p in m.parameters():
        p.grad = None
    q = c["q_ctx"].clone().requires_grad_(True)
    ch = c["chunks"].clone().requires_grad_(True)
    s = selected_window_scores(m, q, ch, c["cmask"], c["slot"], c["qm"], c["win"], c["C"])
    (s * c["go"]).sum().backward()
    params = dict(m.named_parameters())
    worst = 0.0
    for n, got, want in [("grad_q", q.grad, gq64), ("grad_chunks", ch.grad, gc64)] + \
            [(n, params[n].grad.reshape(-1)[:gp64[n].numel()], gp64[n]) for n in gp64]:
        r = T.error_ratio(got, want)
        print(f"[tkl bwd f32/f64] {name} {sat} {n}: |want|max {float(want.abs().max()):.3e} error/bound {r:.4f}")
        assert r <= 1.0, (name, sat, n, r)
        worst = max(worst, r)
    print(f"[tkl bwd f32/f64] {name} {sat} WORST {worst:.4f}")
    for p in m.parameters():
        p.grad = None
    assert sum(float(gp64[n].abs().max()) >= 1.0 for n in gp64) >= 1 and float(gq64.abs().max()) >= 1.0, \
        "the gradients are of order 1: the absolute term of the bound is a relative one"
