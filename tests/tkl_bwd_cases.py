"""TEST INFRASTRUCTURE — inputs and the float64 reference for the tests of mm_tkl_bwd (tests/test_tkl_bwd_cases_cpu.py proves
the table and the bound without a GPU, tests/test_tkl_bwd_routes_gpu.py runs every kernel and launch form on it).

Everything here is built on the CPU from seeded generators, so the CPU module and the GPU module (parent and children) see
the same bits.  The reference is `tests/tkl_window_reference.selected_window_scores` — the differentiable restatement of
sigir20_tkl.py:184-286 on the 15 selected windows, itself pinned on the real class's gradients — on a float64 copy of the
module and of the inputs.  The window scores stay the float32 values, so both sides pick the same regions.

The bound is the project's bound for this backward (tests/test_tkl_gpu.py): |got - want| <= 3e-4 max(1, |want|max) + 2e-3 |want|.
`go` and `dense.weight` are scaled so that the large gradient tensors have |want|max >= 1: the absolute term is then a relative
one, 3e-4 of the largest entry, and not a floor far above the gradients themselves."""
import copy
import functools

import numpy as np
import torch

from matchmaker_amd.tkl import CHUNK, OVERLAP, TKL_sigir20, chunk_documents, region_peaks
from tests.tkl_window_reference import selected_window_scores

MU = [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9]
SIGMA = [0.1] * 11
K = 11
RTOL, ATOL = 2e-3, 3e-4          # x max(1, |want|max): the bound of test_native_backward_equals_the_differentiable_torch_restatement

# the parameters that test names, per saturation, with (offset, length) in the packed vector (TKL_sigir20._pack_layout)
_SAT = 4 * K
LAYOUT = {"dense.weight": (2 * K, K), "kernel_mult": (3 * K, K),
          "saturation_linear.weight": (_SAT, 2), "saturation_linear.bias": (_SAT + 2, 1),
          "saturation_linear2.weight": (_SAT + 3, 2), "saturation_linear2.bias": (_SAT + 5, 1),
          "saturation_linear3.weight": (_SAT + 6, 2), "saturation_linear3.bias": (_SAT + 8, 1),
          "sat_normer.weight": (_SAT + 9, 2), "sat_normer.bias": (_SAT + 11, 2),
          "chunk_scoring": (4 * K + 13, 15), "sat_emb_reduce1.weight": (4 * K + 28, None)}


def param_names(sat):
    return ["dense.weight", "chunk_scoring"] + (
        ["saturation_linear.weight", "saturation_linear.bias", "saturation_linear2.weight", "saturation_linear2.bias",
         "saturation_linear3.weight", "saturation_linear3.bias", "sat_normer.weight", "sat_normer.bias",
         "sat_emb_reduce1.weight"] if sat == "embedding" else ["kernel_mult"])


def named_from_packed(gp, sat, E):
    """The packed parameter gradient [MM_TKL_NPARAMS] of ops.tkl_bwd -> {name: flat slice} for the names of `sat`."""
    out = {}
    for n in param_names(sat):
        lo, cnt = LAYOUT[n]
        out[n] = gp[lo:lo + (E if cnt is None else cnt)]
    return out


def make_model(E, sat, seed):
    """A TKL_sigir20 on the CPU whose saturation parameters are off their init plateau (bias 100, weights +-0.014: there no
    parameter but the bias carries a gradient above rounding), as the existing backward tests move them; dense.weight is drawn
    at N(0, 0.3) instead of +-0.014 so that the gradients are of order 1 (see the module docstring).  Only the scoring
    parameters matter: the tests never run the contextualiser."""
    heads = next(h for h in (10, 8, 4, 2, 1) if E % h == 0)
    torch.manual_seed(seed)                # the constructor draws from the global generator
    m = TKL_sigir20(E, MU, SIGMA, heads, 1, 32, 2000, True, True, sat)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for lin in (m.saturation_linear, m.saturation_linear2, m.saturation_linear3):
            lin.bias.fill_(2.0)
            lin.weight.normal_(0, 0.3, generator=g)
        m.sat_normer.weight.normal_(1.0, 0.2, generator=g)
        m.chunk_scoring.normal_(1.0, 0.3, generator=g)
        m.kernel_mult.normal_(1.0, 0.1, generator=g).abs_()
        m.dense.weight.normal_(0, 0.3, generator=g)
    return m.train()


def reference64(model, q_ctx, chunks, cmask, slot, qm, win, C, go):
    """Autograd through selected_window_scores on a CPU float64 deep copy of `model` and float64 copies of the inputs (`win`
    keeps its float32 VALUES: the same region picks).  Returns (grad_q [B, Q, E], grad_chunks [P, 50, E], {name: flat grad}) in
    float64; a parameter's gradient is flattened and cut to the entries the scoring reads (kernel_mult: the first K of 4 K)."""
    sat = "embedding" if model.use_embedding_sat else "log"
    m = copy.deepcopy(model).cpu().double()
    for p in m.parameters():
        p.grad = None
    f64 = lambda t: t.detach().cpu().double()
    q = f64(q_ctx).requires_grad_(True)
    c = f64(chunks).requires_grad_(True)
    win32 = win.detach().cpu().float()
    assert torch.equal(win32.double().float(), win32)
    s = selected_window_scores(m, q, c, f64(cmask), slot.detach().cpu(), f64(qm), win32.double(), C)
    (s * f64(go)).sum().backward()
    params = dict(m.named_parameters())
    E = q.shape[-1]
    gp = {}
    for n in param_names(sat):
        cnt = LAYOUT[n][1]
        gp[n] = params[n].grad.reshape(-1)[:E if cnt is None else cnt].clone()
    return q.grad, c.grad, gp


def selected_windows(win):
    """[B, 15] window indices in the order of :275-277 (peaks, -1, +1, -2, +2; clamped), from the float32 window scores."""
    top = region_peaks(win.detach().cpu().float())
    W = max(win.shape[1], 3)
    return top, torch.cat([top, top - 1, top + 1, top - 2, top + 2], dim=1).clamp_(0, W - 1)


def structural_zero_rows(win, slot, C):
    """bool [P, 50]: the chunk rows that none of the 15 selected windows of any document reads — the index arithmetic of
    tests/tkl_window_reference.py:24-35 (masks play no part: a padding row inside a window is read, and gets a zero by
    arithmetic).  mm_tkl_bwd must leave exact zeros on these rows."""
    B = win.shape[0]
    slot = slot.detach().cpu().long()
    P = slot.numel()
    _, idx = selected_windows(win)
    t = 2 * idx.unsqueeze(-1) + torch.arange(30)                                   # [B, 15, 30]
    in_doc = t < C * CHUNK
    t = t.clamp(max=C * CHUNK - 1)
    s = torch.arange(B).view(B, 1, 1) * C + t // CHUNK
    slot2p = torch.full((B * C,), -1, dtype=torch.long)
    slot2p[slot] = torch.arange(P)
    p = slot2p[s]
    present = (p >= 0) & in_doc
    row = t % CHUNK + OVERLAP
    read = torch.zeros(P, 50, dtype=torch.bool)
    read[p[present], row[present]] = True
    return ~read


def error_ratio(got, want):
    """max |got - want| / (ATOL max(1, |want|max) + RTOL |want|): <= 1 is inside the bound.  numpy / torch in, float out."""
    got = np.asarray(got.detach().cpu().double() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu().double() if torch.is_tensor(want) else want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    assert np.isfinite(got).all(), "non-finite gradient"
    bound = ATOL * max(1.0, float(np.abs(want).max())) + RTOL * np.abs(want)
    return float((np.abs(got - want) / bound).max())


# ---- the planted cases ------------------------------------------------------------------------------------------------------
# Q = 12, D = 400 (C = 10 chunks, W = 186 windows), E = 64, as test_backward_when_the_regions_overlap_or_sit_at_the_ends builds
# them.  Per document: d_len, mask holes [lo, hi), planted (window, value) pairs on a floor of 0.01 .. 0.11 (0 on windows
# without a token, as the forward leaves them), the picks the region search must make of them and their pairwise distances
# |p0 - p1|, |p1 - p2|, |p0 - p2|.  Window w covers document positions 2 w .. 2 w + 29 and a region the windows p - 2 .. p + 2,
# i.e. positions 2 p - 4 .. 2 p + 33: two regions share 38 - 2 |p - p'| positions (8 at 15 apart, 6 at 16, 2 at 18) and are
# disjoint from 19 apart.
#
# ratio: the largest error / bound of the float32 restatement on the CPU against float64, over grad_q, grad_chunks and every
# parameter (embedding | log saturation), as tests/test_tkl_bwd_cases_cpu.py measures and prints it: a correct float32
# implementation sits this far inside the bound at these inputs.
Q, D, E = 12, 400, 64


def _doc(peaks, picks, d_len=D, holes=()):
    return {"peaks": peaks, "picks": picks, "d_len": d_len, "holes": holes}


def _ranked(*ws):
    return [(w, 5.0 - r) for r, w in enumerate(ws)]


CASES = {
    # three regions that share no position                                                                ratio 0.0151 | 0.0012
    "separate": [_doc(_ranked(30, 90, 150), (30, 90, 150)), _doc(_ranked(100, 20, 170), (100, 20, 170)),
                 _doc(_ranked(60, 10, 120), (60, 10, 120), d_len=333)],
    # peaks exactly 15 windows apart: neighbouring regions share 8 positions; ascending and descending     ratio 0.0030 | 0.0035
    "overlap_15_apart": [_doc(_ranked(10, 25, 40), (10, 25, 40)), _doc(_ranked(100, 85, 70), (100, 85, 70))],
    # 16 apart: the peaks' own windows no longer touch, the regions still share 6 positions                ratio 0.0033 | 0.0026
    "adjacent_16_apart": [_doc(_ranked(10, 26, 42), (10, 26, 42)), _doc(_ranked(100, 84, 68), (100, 84, 68))],
    # the last overlap (18 apart: 2 positions), the first disjoint layout (19 apart: the regions touch), and one region
    # between an overlapping and a separate neighbour                                                      ratio 0.0044 | 0.0016
    "overlap_edge_18_19": [_doc(_ranked(50, 68, 86), (50, 68, 86)), _doc(_ranked(88, 69, 50), (88, 69, 50)),
                           _doc(_ranked(120, 105, 140), (120, 105, 140))],
    # peaks at the first and at the last window: neighbour indices clamp (the same window several times)   ratio 0.0169 | 0.0033
    "ends_clamp": [_doc(_ranked(0, 15, 185), (0, 15, 185)), _doc(_ranked(184, 169, 3), (184, 169, 3), d_len=390)],
    # two peaks tied in value: the first arg-max wins.  Across wavefronts (40 | 120, 66 | 130: the rank decides which
    # chunk_scoring weight a window gets) and inside one (40 | 50: the loser is suppressed, not picked)    ratio 0.0039 | 0.0014
    "tied_peaks": [_doc([(40, 5.0), (120, 5.0), (80, 4.0)], (40, 120, 80)),
                   _doc([(40, 5.0), (50, 5.0), (100, 4.0), (130, 3.0)], (40, 100, 130)),
                   _doc([(130, 5.0), (66, 5.0), (20, 4.0)], (66, 130, 20))],
    # a document shorter than one window (29 tokens: windows 0 .. 14 hold a token, every other window is empty).  The second
    # and third picks are then the first empty windows left, 15 and 30; the neighbours 13 and 14 of the second are not empty
    # and share rows with the first region                                                                 ratio 0.0355 | 0.0026
    "shorter_than_a_window": [_doc([(0, 5.0)], (0, 15, 30), d_len=29), _doc(_ranked(30, 90, 150), (30, 90, 150))],
    # a document of one token (window 0 alone), one of two tokens                                          ratio 0.0070 | 0.0018
    "one_token": [_doc([(0, 5.0)], (0, 15, 30), d_len=1), _doc([(0, 5.0)], (0, 15, 30), d_len=2),
                  _doc(_ranked(100, 20, 170), (100, 20, 170))],
    # a middle chunk emptied by a mask hole (tokens 160 .. 199 = chunk 4, dropped from the packed chunks) with a peak on either
    # edge of it; two chunks emptied (80 .. 159) with a peak whose window starts in the last two tokens before the hole and one
    # whose window starts on the first token behind it                                                     ratio 0.0131 | 0.0013
    "hole_empties_a_chunk": [_doc(_ranked(72, 95, 20), (72, 95, 20), holes=((160, 200),)),
                             _doc(_ranked(39, 80, 150), (39, 80, 150), holes=((80, 160),))],
}


@functools.lru_cache(maxsize=None)
def planted(name, sat):
    """The inputs of case `name` on the CPU: dict(model, q_ctx, chunks, cmask, slot, qm, win, C, go, B, picks).  Cached: do not
    modify the tensors."""
    docs = CASES[name]
    B = len(docs)
    seed = 1000 + sorted(CASES).index(name)
    g = torch.Generator().manual_seed(seed)
    m = make_model(E, sat, seed)
    q = torch.randn(B, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    qm = torch.ones(B, Q)
    qm[B - 1, 9:] = 0
    dm = torch.zeros(B, D)
    for b, doc in enumerate(docs):
        dm[b, :doc["d_len"]] = 1
        for lo, hi in doc["holes"]:
            dm[b, lo:hi] = 0
        t = min(2 * doc["picks"][0] + 3, doc["d_len"] - 1)
        d[b, t] = q[b, 1] * 1.5                                  # a planted match in the first region: the high-mu kernels are active
    go = torch.randn(B, generator=g) * 8
    q_ctx = q * qm.unsqueeze(-1)
    chunks, cmask, slot, C = chunk_documents(d * dm.unsqueeze(-1), dm)
    W = (C * CHUNK - 30) // 2 + 1
    pos = 2 * torch.arange(W).unsqueeze(1) + torch.arange(30)                     # [W, 30]
    dm_pad = torch.nn.functional.pad(dm, (0, C * CHUNK + 30 - D))
    nonempty = dm_pad[:, pos].sum(-1) > 0                                         # [B, W]
    win = (torch.rand(B, W, generator=g) * 0.1 + 0.01) * nonempty
    for b, doc in enumerate(docs):
        for w, v in doc["peaks"]:
            assert nonempty[b, w], (name, b, w)
            win[b, w] = v
    return {"model": m, "q_ctx": q_ctx, "chunks": chunks, "cmask": cmask, "slot": slot, "qm": qm, "win": win, "C": C, "go": go,
            "B": B, "sat": sat, "picks": [doc["picks"] for doc in docs]}


@functools.lru_cache(maxsize=None)
def planted_reference(name, sat):
    """(grad_q, grad_chunks, {name: grad}) of case `name` in float64, computed once."""
    c = planted(name, sat)
    return reference64(c["model"], c["q_ctx"], c["chunks"], c["cmask"], c["slot"], c["qm"], c["win"], c["C"], c["go"])


def natural(Qn, Dn, En, sat, B=3, seed=0):
    """Random documents for the tests that take the window scores from the forward: ragged q_len and d_len, document 0 at full
    length, one mask hole inside a chunk (it empties none), a planted match.  dict as planted(), without win and picks."""
    g = torch.Generator().manual_seed(7919 * Qn + 31 * Dn + En + seed)
    m = make_model(En, sat, 50 + seed)
    q = torch.randn(B, Qn, En, generator=g)
    d = torch.randn(B, Dn, En, generator=g)
    ql = torch.randint(1, Qn + 1, (B,), generator=g)
    ql[0] = Qn
    dl = torch.randint(Dn // 3 + 1, Dn + 1, (B,), generator=g)
    dl[0] = Dn
    if B > 1:
        dl[1] = max(1, min(int(dl[1]), Dn - 1))
    qm = (torch.arange(Qn)[None] < ql[:, None]).float()
    dm = (torch.arange(Dn)[None] < dl[:, None]).float()
    dm[0, 12:19] = 0                                             # inside chunk 0 (tokens 0 .. 39)
    d[0, 7] = q[0, min(1, Qn - 1)] * 1.5
    go = torch.randn(B, generator=g) * 8
    q_ctx = q * qm.unsqueeze(-1)
    chunks, cmask, slot, C = chunk_documents(d * dm.unsqueeze(-1), dm)
    return {"model": m, "q_ctx": q_ctx, "chunks": chunks, "cmask": cmask, "slot": slot, "qm": qm, "C": C, "go": go, "B": B, "sat": sat}


# ---- shapes for the tests that take the window scores from the forward --------------------------------------------------------
# (Q, D, E) -> the kernel mm_tkl_bwd's dispatch reaches (tkl_bwd.hip, host entry): tiled<5> for E <= 320, tiled<8> for
# 320 < E <= 512 while tkl_bwd_tiled_lds_bytes(Wp, Q, E) <= 150 KiB, the per-element kernel otherwise.
NATURAL = [((7, 120, 64), "tiled<5>"), ((20, 333, 300), "tiled<5>"), ((1, 41, 8), "tiled<5>"),
           ((16, 300, 324), "tiled<8>"), ((12, 160, 512), "tiled<8>"),
           ((9, 120, 520), "per-element"), ((20, 160, 768), "per-element"),
           # Q = 32, E = 512, W = 46: the tiled kernel would need 188,416 bytes of LDS (131,936 at Q = 12, D = 160) > 153,600
           ((32, 120, 512), "per-element")]
