"""GPU tests of the native training losses (csrc/losses.hip through matchmaker_amd/losses.py).

Yardstick: the float64 restatement (tests/losses_reference.py).  Per case e_ref = the error of the reference's own fp32 result
against it (the module's eager formula in fp32 on CPU, which tests/test_losses_cpu.py holds to the reference classes); the
device must be within 4 e_ref + 4 fp32 ulps, the ulp taken of |loss| for the loss and of the list's (or vector's) largest
|gradient| for gradients.  16-bit gradients: within one 16-bit ulp of the rounded float64 gradient.

Shapes: pairs n in {1, 63, 64, 65, 1025, 70,000} (the last is more than one workgroup's share: the partial-sum pass runs);
lists L in {1, 2, 63, 64, 65, 130, 1024} x B in {1, 5, 33} in fp32 (both kernel forms, B no multiple of four), and every L at
B = 5 in fp16 and bf16 (the dtype changes the load and the store only, neither depends on B), plus B = 1 and 33 at L = 64 and
130 for one kind.  Scores are 2 N(0, 1) clipped
to +-6.8: 1,024 draws span more than 13.8 now and then, and the clip keeps every gap below it, so the clamp at p = 1e-6 is
reached by the planted case only.  The input conditions are asserted on the CPU inside each test.
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from matchmaker_amd import losses, ops
from tests import losses_reference as R, poison, util

pytestmark = pytest.mark.gpu

PAIR_N = (1, 63, 64, 65, 1025, 70000)
LIST_L = (1, 2, 63, 64, 65, 130, 1024)
LIST_B = (1, 5, 33)
DT16 = (torch.float16, torch.bfloat16)
LN_EPS = math.log(1e-6)
CLASS = {"ranknet": losses.RankNetLoss, "margin": losses.MarginRankingLoss1, "margin_mse": losses.MSMarginLoss,
         "mse_pointwise": losses.MSETeacherPointwise, "kldiv_pointwise": losses.KLDivTeacherPointwise,
         "ranknet_teacher": losses.RankNetTeacher, "mse_ranknet": losses.MSERanknetTeacher, "listnet": losses.ListNetLoss,
         "kldiv": losses.KLDivTeacherList, "smooth_mrr": losses.SmoothMRRLoss,
         "lambda_ndcg2": lambda: losses.LambdaLoss("ndcgLoss2_scheme"),
         "lambda_ndcg2_teacher": lambda: losses.LambdaLossTeacher("ndcgLoss2_scheme")}


def seed_of(*key):
    return zlib.crc32("|".join(map(str, key)).encode())


def widen(x32, dtype):
    """fp32 numpy values rounded to `dtype` and widened back (exactly what the kernel reads)"""
    return torch.from_numpy(x32).to(dtype).to(torch.float32).numpy()


# ---- inputs and references, computed once per case and never modified ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_case(kind, n, dtype=torch.float32):
    rng = np.random.default_rng(seed_of("pair", kind, n))
    f = np.float32
    pos, neg = f(np.clip(2 * rng.standard_normal(n), -6.8, 6.8)), f(np.clip(2 * rng.standard_normal(n), -6.8, 6.8))
    if dtype != torch.float32:
        pos, neg = widen(pos, dtype), widen(neg, dtype)
    if kind == "ranknet":
        labels = (f(rng.random(n)),)
    elif kind == "margin":
        labels = (f(rng.choice([-1.0, 1.0], n)),)
        kink = 1.0 - labels[0].astype(np.float64) * (pos.astype(np.float64) - neg) == 0      # (16-bit scores differ by exactly 1 often)
        neg[kink] += np.float32(0.5)                  # still a 16-bit value; the kink has its own test
        assert not np.any(1.0 - labels[0].astype(np.float64) * (pos.astype(np.float64) - neg) == 0)
    else:
        labels = (f(np.abs(rng.standard_normal(n)) + 0.1), f(np.abs(rng.standard_normal(n)) + 0.1))
    ref64 = R.pair(kind, pos, neg, *labels)
    p, g = torch.from_numpy(pos).requires_grad_(), torch.from_numpy(neg).requires_grad_()
    loss = CLASS[kind]().eager(p, g, *[torch.from_numpy(t) for t in labels])
    loss.backward()
    ref32 = (loss.detach().numpy(), p.grad.numpy(), g.grad.numpy())
    for a in (pos, neg) + labels:
        a.setflags(write=False)
    return pos, neg, labels, ref64, ref32


def list_inputs(kind, B, L, dtype, salt=0):
    rng = np.random.default_rng(seed_of("list", kind, B, L, salt))
    f = np.float32
    scores = f(np.clip(2 * rng.standard_normal((B, L)), -6.8, 6.8))
    if dtype != torch.float32:
        scores = widen(scores, dtype)
    if kind == "lambda_ndcg2":
        labels = f(rng.integers(0, 4, (B, L)))
        labels[0, L // 2 + 1:] = -1               # some padded (none when L <= 2: list 0 is then whole)
        if B > 1:
            labels[1, 1:] = -1                    # all but one
        if B > 2:
            labels[2, :] = -1                     # fully padded: term 0, gradient all zeros
    elif kind == "smooth_mrr":
        labels = f(rng.random((B, L)) < 0.3)
        labels[:, 0] = 1
        if B > 2:
            labels[2, :] = 0                      # no relevant entry: term 1, gradient all zeros
    else:
        labels = f(3 * rng.standard_normal((B, L)))
        for _ in range(50 if kind == "lambda_ndcg2_teacher" else 0):
            # among 1,024 softmax values some always lie near the 0.001 threshold: those teacher scores are moved by 0.25
            near = np.abs(R.teacher_labels(labels)[1].astype(np.float64) - 0.001) <= 2e-5
            if not near.any():
                break
            labels[near] += f(0.25)
    return scores, labels


def assert_list_conditions(kind, scores, labels):
    s = scores.astype(np.float64)
    assert (s.max(-1) - s.min(-1)).max() < 13.8
    if kind == "smooth_mrr":
        rr = np.sort(np.where(labels > 0, R.smooth_mrr_rr(scores), 0.0), axis=-1)
        if rr.shape[1] > 1:
            assert np.all((rr[:, -1] - rr[:, -2] > 1e-4) | (rr[:, -1] == 0)), "best and second-best rr closer than 1e-4"
    if kind.startswith("lambda"):
        y = labels.astype(np.float64)
        if kind == "lambda_ndcg2_teacher":
            y, T = R.teacher_labels(labels)
            assert np.abs(T.astype(np.float64) - 0.001).min() > 1e-5, "a teacher-softmax label within 1e-5 of 0.001"
        for r in range(s.shape[0]):
            x = R.lambda_pairs(s[r], y[r])[3]
            assert x.size == 0 or np.abs(x - LN_EPS).min() >= 1e-3, "a counted pair within 1e-3 of the clamp"


@functools.lru_cache(maxsize=None)
def list_case(kind, B, L, dtype=torch.float32):
    for salt in range(20):      # the first seed whose INPUTS meet the conditions (no device result is involved)
        scores, labels = list_inputs(kind, B, L, dtype, salt)
        try:
            assert_list_conditions(kind, scores, labels)
            break
        except AssertionError:
            if salt == 19:
                raise
    ref64 = R.lists(kind, scores, labels)
    s = torch.from_numpy(scores).requires_grad_()
    mod = CLASS[kind]()
    loss = mod.eager(s, torch.from_numpy(labels))
    loss.backward()
    ref32 = [loss.detach().numpy(), s.grad.numpy()]
    with torch.no_grad():      # the reference's own fp32 per-list terms: the formula on each list alone (a mean / a sum over one list)
        ref32.append(np.array([float(mod.eager(torch.from_numpy(scores[r:r + 1]), torch.from_numpy(labels[r:r + 1]))) for r in range(B)]))
    scores.setflags(write=False)
    labels.setflags(write=False)
    return scores, labels, ref64, ref32


def dev_t(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.array(x)).to(dev).to(dtype)


def check(label, got, ref32, ref64, per_row=False):
    """|got - ref64| <= 4 e_ref + 4 fp32 ulps (of |loss|, or of the largest |gradient| of the vector / of each list); the
    figures are printed before the assertion"""
    got, ref32, ref64 = R.f64(got), R.f64(ref32), R.f64(ref64)
    if per_row and got.ndim == 1:      # one value per list
        got, ref32, ref64 = got[:, None], ref32[:, None], ref64[:, None]
    if not per_row:
        got, ref32, ref64 = got.reshape(1, -1), ref32.reshape(1, -1), ref64.reshape(1, -1)
    err = np.abs(got - ref64).max(-1)
    e_ref = np.abs(ref32 - ref64).max(-1)
    ulp = R.ulp32(np.abs(ref64).max(-1))
    lim = 4 * e_ref + 4 * ulp
    worst = int(np.argmax(err - lim))
    print(f"{label}: err {err[worst]:.3e} ({err[worst] / ulp[worst]:.2f} ulp) e_ref {e_ref[worst]:.3e} bound {lim[worst]:.3e}")
    assert np.all(err <= lim), f"{label}: row {worst}: error {err[worst]:.3e} above 4 e_ref + 4 ulp = {lim[worst]:.3e}"


def check16(label, got, ref64, dtype):
    want = R.round16(ref64, dtype)
    err = np.abs(R.f64(got.float().cpu().numpy()) - want)
    lim = R.ulp16(want, dtype)
    print(f"{label}: worst {np.max(err / lim):.2f} 16-bit ulp")
    assert np.all(err <= lim), label


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PAIR_N)
@pytest.mark.parametrize("kind", R.PAIR_KINDS)
def test_pair_accuracy(kind, n):
    dev = util.require_gpu()
    for dtype in (torch.float32,) + DT16:
        pos, neg, labels, ref64, ref32 = pair_case(kind, n, dtype)
        lab = [dev_t(t, dev) for t in labels] + [None] * (2 - len(labels))
        loss, gp, gn = losses.pair_loss(dev_t(pos, dev, dtype), dev_t(neg, dev, dtype), lab[0], lab[1], kind)
        assert loss.dtype == torch.float32 and loss.shape == () and gp.dtype == gn.dtype == dtype
        tag = f"{kind} n={n} {dtype}"
        check(tag + " loss", loss.item(), ref32[0], ref64[0])
        if dtype == torch.float32:
            check(tag + " gpos", gp.cpu().numpy(), ref32[1], ref64[1])
            check(tag + " gneg", gn.cpu().numpy(), ref32[2], ref64[2])
        else:
            check16(tag + " gpos", gp, ref64[1], dtype)
            check16(tag + " gneg", gn, ref64[2], dtype)


def _list_check(kind, B, L, dtype, dev):
    scores, labels, ref64, ref32 = list_case(kind, B, L, dtype)
    loss, per, grad = losses.list_loss(dev_t(scores, dev, dtype), dev_t(labels, dev), kind)
    assert loss.shape == () and per.shape == (B,) and grad.shape == (B, L) and grad.dtype == dtype
    tag = f"{kind} B={B} L={L} {dtype}"
    check(tag + " loss", loss.item(), ref32[0], ref64[0])
    per_np = per.cpu().numpy()
    check(tag + " per_list", per_np, ref32[2], ref64[1], per_row=True)
    denom = 1.0 if kind.startswith("lambda") else float(B)      # the finishing launch: float64 sum of per_list, one rounding
    assert abs(per_np.astype(np.float64).sum() / denom - loss.item()) <= R.ulp32(loss.item())
    if dtype == torch.float32:
        check(tag + " grad", grad.cpu().numpy(), ref32[1], ref64[2], per_row=True)
    else:
        check16(tag + " grad", grad, ref64[2], dtype)
    if kind == "lambda_ndcg2" and B > 2:
        assert per_np[2] == 0 and not grad[2].float().cpu().numpy().any(), "the fully padded list: term 0, gradient all zeros"
        assert not grad.float().cpu().numpy()[labels == -1].any(), "padded entries get gradient 0"


@pytest.mark.parametrize("B", LIST_B)
@pytest.mark.parametrize("L", LIST_L)
@pytest.mark.parametrize("kind", R.LIST_KINDS)
def test_list_accuracy_fp32(kind, L, B):
    _list_check(kind, B, L, torch.float32, util.require_gpu())


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("L", LIST_L)
@pytest.mark.parametrize("kind", R.LIST_KINDS)
def test_list_accuracy_16bit(kind, L, dtype):
    _list_check(kind, 5, L, dtype, util.require_gpu())


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def bits32(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ("margin_mse", "mse_pointwise"))
def test_small_integers_are_bit_exact(kind):
    dev = util.require_gpu()
    rng = np.random.default_rng(3)
    n = 64
    pos, neg, a, b = (np.float32(rng.integers(-8, 9, n)) for _ in range(4))
    loss, gp, gn = losses.pair_loss(dev_t(pos, dev), dev_t(neg, dev), dev_t(a, dev), dev_t(b, dev), kind)
    l64, gp64, gn64 = R.pair(kind, pos, neg, a, b)
    assert bits32(loss.item()) == bits32(l64)
    assert np.array_equal(bits32(gp.cpu().numpy()), bits32(gp64)) and np.array_equal(bits32(gn.cpu().numpy()), bits32(gn64))


def test_margin_at_the_kink_passes_the_gradient():
    dev = util.require_gpu()
    pos = np.float32([3, 2, 0.5, -1, 4, 0, 1, 1])
    neg = np.float32([2, 3, 0.25, 1, 0, 4, 1, 0])
    y = np.float32([1, -1, 1, 1, 1, 1, -1, 1])      # x = 1, -1 (kink for y = 1, -1), .25, -2, 4, -4, 0, 1 (kink)
    h = 1.0 - y.astype(np.float64) * (pos.astype(np.float64) - neg)
    assert list(h == 0) == [True, True, False, False, False, False, False, True]
    loss, gp, gn = losses.pair_loss(dev_t(pos, dev), dev_t(neg, dev), dev_t(y, dev), None, "margin")
    l64, gp64, gn64 = R.pair("margin", pos, neg, y)
    assert bits32(loss.item()) == bits32(l64)
    assert np.array_equal(bits32(gp.cpu().numpy()), bits32(gp64)) and np.array_equal(bits32(gn.cpu().numpy()), bits32(gn64))
    assert gp.cpu().numpy()[0] == np.float32(-1 / 8) and gp.cpu().numpy()[1] == np.float32(1 / 8) and gp.cpu().numpy()[4] == 0


def eager_cpu(kind, scores, labels):
    """(loss, grad) of the module's eager formula in fp32 on the CPU: the reference's own fp32 result, the e_ref of check()"""
    s = torch.from_numpy(np.array(scores)).requires_grad_()
    loss = CLASS[kind]().eager(s, torch.from_numpy(np.array(labels)))
    loss.backward()
    return loss.item(), s.grad.numpy()


# The three list cases below are NOT bit-equal to the rounded float64 restatement (the issue expected that of all five exact
# cases): the list kinds form their terms in fp32, and a logarithm or a sigmoid has no exact fp32 value.  What is exact is
# asserted exactly (a gradient of 0, the tie order, the arg-max index); the values are held to the general rule, 4 e_ref + 4 fp32
# ulps, with e_ref from the eager formula on the CPU, whose sort is stable.  DESIGN 3.22 names this as a departure.
def test_lambda_planted_gap_of_20_is_clamped():
    dev = util.require_gpu()
    # two entries: the higher label scores 20 below the other, so p = sigmoid(-20) < 1e-6: term = -log2(1e-6^w), gradient exactly 0
    scores, labels = np.float32([[0, 20]]), np.float32([[1, 0]])
    ii, jj, w, x, _ = R.lambda_pairs(scores[0], labels[0])
    assert x.tolist() == [-20.0]
    l32, g32 = eager_cpu("lambda_ndcg2", scores, labels)
    loss, per, grad = losses.list_loss(dev_t(scores, dev), dev_t(labels, dev), "lambda_ndcg2")
    want = -np.log2(R.EPS ** w[0])
    assert np.isclose(want, R.lists("lambda_ndcg2", scores, labels)[0], rtol=1e-14) and not g32.any()
    assert np.array_equal(bits32(grad.cpu().numpy()), bits32([[0, 0]]))
    check("planted pair loss", loss.item(), l32, want)
    assert per.cpu().numpy()[0] == np.float32(loss.item())
    # ... and inside a longer list next to live pairs
    scores = np.float32([[0.5, -20, 0, 0.25, -1], [1, 2, 3, 4, 5]])
    labels = np.float32([[0, 3, 1, 2, -1], [0, 1, 0, 2, 1]])
    assert R.lambda_pairs(scores[0], labels[0])[3].min() == -20.5
    l32, g32 = eager_cpu("lambda_ndcg2", scores, labels)
    l64, _, g64 = R.lists("lambda_ndcg2", scores, labels)
    loss, per, grad = losses.list_loss(dev_t(scores, dev), dev_t(labels, dev), "lambda_ndcg2")
    check("planted loss", loss.item(), l32, l64)
    check("planted grad", grad.cpu().numpy(), g32, g64, per_row=True)
    assert grad.cpu().numpy()[0, 4] == 0


def test_exactly_tied_scores_follow_the_stable_rule():
    dev = util.require_gpu()
    scores = np.float32([[1, 1, 0, 1, -0.0, 2]])
    labels = np.float32([[0, 2, 1, 3, 0, 1]])
    l64, _, g64 = R.lists("lambda_ndcg2", scores, labels)
    # the case discriminates: the reversed arrival order among the ties gives another loss
    alt = scores.astype(np.float64) + np.float64([[0, 1e-9, 0, 2e-9, 1e-9, 0]])
    assert abs(R.lists("lambda_ndcg2", alt, labels)[0] - l64) > 1e-3
    l32, g32 = eager_cpu("lambda_ndcg2", scores, labels)      # (the eager formula sorts with stable=True: the same order)
    assert abs(l32 - l64) < 1e-4
    loss, per, grad = losses.list_loss(dev_t(scores, dev), dev_t(labels, dev), "lambda_ndcg2")
    check("tied loss", loss.item(), l32, l64)
    check("tied grad", grad.cpu().numpy(), g32, g64, per_row=True)


def test_smooth_mrr_tied_best_takes_the_lowest_index():
    dev = util.require_gpu()
    scores, labels = np.float32([[1, 1, 0, -1], [0, 2, 2, 1]]), np.float32([[1, 1, 0, 0], [0, 1, 1, 1]])
    rr = np.where(labels > 0, R.smooth_mrr_rr(scores), 0)
    assert rr[0, 0] == rr[0, 1] == rr[0].max() and rr[1, 1] == rr[1, 2] == rr[1].max()
    l64, per64, g64 = R.lists("smooth_mrr", scores, labels)
    l32, g32 = eager_cpu("smooth_mrr", scores, labels)
    loss, per, grad = losses.list_loss(dev_t(scores, dev), dev_t(labels, dev), "smooth_mrr")
    g = grad.cpu().numpy()
    assert g[0, 0] < 0 < g[0, 1] and g[1, 1] < 0 < g[1, 2], "the gradient flows through the lowest tied index"
    check("tied rr loss", loss.item(), l32, l64)
    if g32[0, 0] < 0 < g32[0, 1] and g32[1, 1] < 0 < g32[1, 2]:      # torch's max took the lowest index too: its error is the e_ref
        check("tied rr grad", g, g32, g64, per_row=True)
    else:                                                            # (its arg-max on ties is open: then no e_ref, 4 ulps alone)
        check("tied rr grad", g, g64, g64, per_row=True)


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("B", (1, 33))
@pytest.mark.parametrize("L", (64, 130))
def test_list_accuracy_16bit_other_batch_sizes(L, B, dtype):
    """the rest of the L x B x dtype grid for one kind per kernel form (64: one wavefront per list, 130: one workgroup)"""
    _list_check("lambda_ndcg2", B, L, dtype, util.require_gpu())


# ---- autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PAIR_KINDS + R.LIST_KINDS)
def test_autograd_through_the_drop_in_class(kind):
    dev = util.require_gpu()
    pairwise = kind in R.PAIR_KINDS
    if pairwise:
        pos, neg, labels = pair_case(kind, 65)[:3]
        scores = [dev_t(pos, dev).requires_grad_(), dev_t(neg, dev).requires_grad_()]
        labels = [dev_t(t, dev) for t in labels]
        saved = losses.pair_loss(scores[0], scores[1], labels[0], labels[1] if len(labels) > 1 else None, kind)[1:]
    else:
        s, y = list_case(kind, 5, 65)[:2]
        scores, labels = [dev_t(s, dev).requires_grad_()], [dev_t(y, dev)]
        saved = losses.list_loss(scores[0], labels[0], kind)[2:]
    before = [poison.bits(t).clone() for t in scores + labels]
    mod = CLASS[kind]()
    mod.native = True      # (the route under test; two classes default to the eager one)
    loss = mod(*scores, *labels)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    for t, g in zip(scores, saved):
        assert torch.equal(poison.bits(t.grad), poison.bits(g)), "backward = the saved gradient x 1"
        t.grad = None
    (mod(*scores, *labels) * 1024.0).backward()
    for t, g in zip(scores, saved):
        assert torch.equal(poison.bits(t.grad), poison.bits(g * 1024.0)), "backward = 1024 x the saved gradient, exactly"
    assert all(t.grad is None for t in labels), "labels get no gradient"
    for t, b in zip(scores + labels, before):
        assert torch.equal(poison.bits(t), b), "inputs are bit-unchanged"


def test_smooth_mrr_agg_false_is_per_list_and_differentiable():
    dev = util.require_gpu()
    s, y, ref64, ref32 = list_case("smooth_mrr", 5, 65)
    scores, labels = dev_t(s, dev).requires_grad_(), dev_t(y, dev)
    assert losses.SmoothMRRLoss.native is True
    per = losses.SmoothMRRLoss()(scores, labels, agg=False)
    check("agg=False", per.detach().cpu().numpy(), ref32[2], ref64[1], per_row=True)
    per.mean().backward()
    check("agg=False grad", scores.grad.cpu().numpy(), ref32[1], ref64[2], per_row=True)


def test_torch_ops_have_the_same_autograd():
    dev = util.require_gpu()
    import matchmaker_amd.torch_ops  # noqa: F401
    pos, neg, labels = pair_case("margin_mse", 65)[:3]
    p, n = dev_t(pos, dev).requires_grad_(), dev_t(neg, dev).requires_grad_()
    loss, gp, gn = torch.ops.mm_native.pair_loss(p, n, dev_t(labels[0], dev), dev_t(labels[1], dev), losses.PAIR_KINDS["margin_mse"])
    assert not gp.requires_grad and not gn.requires_grad
    (loss * 2.0).backward()
    assert torch.equal(p.grad, gp * 2.0) and torch.equal(n.grad, gn * 2.0)
    s, y = list_case("listnet", 5, 65)[:2]
    sc = dev_t(s, dev).requires_grad_()
    loss, per, grad = torch.ops.mm_native.list_loss(sc, dev_t(y, dev), losses.LIST_KINDS["listnet"])
    assert not grad.requires_grad
    loss.backward()
    assert torch.equal(sc.grad, grad)


# ---- determinism and capture ------------------------------------------------------------------------------------------------------
CAPTURE = [("pair", "mse_ranknet", 65, 0), ("pair", "ranknet_teacher", 70000, 0), ("list", "lambda_ndcg2", 5, 17),
           ("list", "lambda_ndcg2_teacher", 5, 130), ("list", "smooth_mrr", 5, 65), ("list", "listnet", 5, 64)]


def _call_case(form, kind, a, b, dev):
    if form == "pair":
        pos, neg, labels = pair_case(kind, a)[:3]
        args = (dev_t(pos, dev), dev_t(neg, dev), dev_t(labels[0], dev), dev_t(labels[1], dev))
        return lambda: losses.pair_loss(*args, kind)
    s, y = list_case(kind, a, b)[:2]
    args = (dev_t(s, dev), dev_t(y, dev))
    return lambda: losses.list_loss(*args, kind)


@pytest.mark.parametrize("form,kind,a,b", CAPTURE)
def test_two_calls_and_a_captured_replay_give_the_same_bits(form, kind, a, b):
    dev = util.require_gpu()
    fn = _call_case(form, kind, a, b, dev)
    first, second = fn(), fn()
    poison.assert_same_bits(first, second, "two calls")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up off the default stream, as torch.cuda.graph asks
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # one stream, one linear chain of launches: no parallel branches
        out = fn()
    for t in out:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    poison.assert_same_bits(first, out, "captured replay")


# ---- poisoned memory --------------------------------------------------------------------------------------------------------------
POISON = [("pair", "mse_ranknet", 65, 0), ("pair", "margin_mse", 70000, 0), ("list", "lambda_ndcg2", 5, 17), ("list", "lambda_ndcg2", 5, 130),
          ("list", "listnet", 5, 64), ("list", "kldiv", 5, 65)]


@pytest.mark.parametrize("form,kind,a,b", POISON)
def test_every_output_is_written_whatever_the_memory_held(form, kind, a, b):
    dev = util.require_gpu()
    fn = _call_case(form, kind, a, b, dev)
    if kind == "lambda_ndcg2":
        assert (list_case(kind, a, b)[1] == -1).any(), "the padded-entry case"
    outs = []
    for p in poison.POISONS:
        out, arena = poison.run(fn, p, module=losses, label=f"{form} {kind} {a} {b}")
        assert len(arena.allocations) == (3 + (1 if form == "pair" and a > 4096 else 0)), "outputs (and the workspace) came from the arena"
        outs.append(out)
    poison.assert_same_bits(outs[0], outs[1], f"{form} {kind} {a} {b}")
    poison.assert_same_bits(outs[0], fn(), "against an unpoisoned call")


# ---- routes ---------------------------------------------------------------------------------------------------------------------
def test_a_list_of_1025_takes_the_eager_path():
    dev = util.require_gpu()
    rng = np.random.default_rng(8)
    scores, labels = np.float32(np.clip(2 * rng.standard_normal((2, 1025)), -6.8, 6.8)), np.float32(3 * rng.standard_normal((2, 1025)))
    with pytest.raises(losses.NativeError) as e:
        losses.list_loss(dev_t(scores, dev), dev_t(labels, dev), "listnet")
    assert e.value.code == losses._lib.MM_EUNSUPPORTED
    for kind in ("listnet", "lambda_ndcg2_teacher"):
        s = dev_t(scores, dev).requires_grad_()
        loss = CLASS[kind]()(s, dev_t(labels, dev))
        assert loss.grad_fn is not None and "ListLoss" not in type(loss.grad_fn).__name__
        loss.backward()
        l64, _, g64 = R.lists(kind, scores, labels)
        # torch's eager fp32 chain on the device (p^w next to 1, then log2): the reference's own kind of error, not bounded by
        # a CPU run's e_ref; 1e-4 relative tells the eager formula from a wrong one, which is what a route test asks
        assert abs(loss.item() - l64) <= 1e-4 * abs(l64) and np.abs(s.grad.cpu().numpy() - g64).max() <= 1e-4 * np.abs(g64).max()


@pytest.mark.parametrize("kind", R.PAIR_KINDS + R.LIST_KINDS)
def test_native_false_and_true_agree(kind):
    dev = util.require_gpu()
    if kind in R.PAIR_KINDS:
        pos, neg, labels, ref64, ref32 = pair_case(kind, 1025)
        scores, labels = [pos, neg], list(labels)
        l64, g64 = ref64[0], ref64[1:]
    else:
        s, y, ref64, ref32 = list_case(kind, 5, 130)
        scores, labels, l64, g64 = [s], [y], ref64[0], [ref64[2]]
    got = {}
    for native in (False, True):
        mod = CLASS[kind]().to(dev)      # (SmoothMRRLoss keeps its 0 / 1 as parameters, as the reference does)
        mod.native = native
        leaves = [dev_t(t, dev).requires_grad_() for t in scores]
        loss = mod(*leaves, *[dev_t(t, dev) for t in labels])
        assert (type(loss.grad_fn).__name__ in ("_PairLossBackward", "_ListLossBackward")) == native, type(loss.grad_fn).__name__
        loss.backward()
        got[native] = (loss.item(), [t.grad.cpu().numpy() for t in leaves])
    # the eager route on the device stands in for the fp32 reference: both within 4 e_ref + 4 ulps of float64
    check(kind + " loss", got[True][0], got[False][0], l64)
    for gn, ge, g in zip(got[True][1], got[False][1], g64):
        check(kind + " grad", gn, ge, g, per_row=gn.ndim == 2)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_colbert_step_with_the_native_margin_mse():
    """64 pairs, Q 32 / D 180 / E 128, bf16: MaxSim forward -> MSMarginLoss -> backward, native loss against eager loss.  The
    float64 of the chain: d loss / d score in float64 from the step's own scores, rounded to fp32 and propagated through
    mm_maxsim_bwd; q.grad and d.grad of both steps must lie within one bf16 ulp of it (the 16-bit gradient rule), and the
    loss and d loss / d score within 4 e_ref + 4 ulps."""
    dev = util.require_gpu()
    import matchmaker_amd.torch_ops  # noqa: F401
    g = torch.Generator().manual_seed(5)
    B, Q, D, E = 64, 32, 180, 128
    q = (torch.randn(B, Q, E, generator=g) / E ** 0.5).to(dev).to(torch.bfloat16)
    dp = (torch.randn(B, D, E, generator=g) / E ** 0.5).to(dev).to(torch.bfloat16)
    dn = (torch.randn(B, D, E, generator=g) / E ** 0.5).to(dev).to(torch.bfloat16)
    tp, tn = (3 * torch.randn(B, generator=g)).to(dev), (3 * torch.randn(B, generator=g)).to(dev)
    steps = {}
    for native in (False, True):
        mod = losses.MSMarginLoss()
        mod.native = native
        leaves = [t.clone().requires_grad_() for t in (q, dp, dn)]
        sp = torch.ops.mm_native.maxsim(leaves[0], leaves[1], None, None)
        sn = torch.ops.mm_native.maxsim(leaves[0], leaves[2], None, None)
        sp.retain_grad(), sn.retain_grad()
        loss = mod(sp, sn, tp, tn)
        loss.backward()
        steps[native] = (loss.item(), sp.detach(), sn.detach(), sp.grad, sn.grad, [t.grad for t in leaves])
    assert torch.equal(steps[True][1], steps[False][1]) and torch.equal(steps[True][2], steps[False][2])
    sp, sn = steps[True][1].cpu().numpy(), steps[True][2].cpu().numpy()
    l64, gp64, gn64 = R.pair("margin_mse", sp, sn, tp.cpu().numpy(), tn.cpu().numpy())
    check("step loss", steps[True][0], steps[False][0], l64)
    check("step d loss / d pos", steps[True][3].cpu().numpy(), steps[False][3].cpu().numpy(), gp64)
    check("step d loss / d neg", steps[True][4].cpu().numpy(), steps[False][4].cpu().numpy(), gn64)
    gq_p, gd_p = ops.maxsim_bwd(q, dp, None, None, dev_t(np.float32(gp64), dev), grad_dtype=torch.bfloat16)
    gq_n, gd_n = ops.maxsim_bwd(q, dn, None, None, dev_t(np.float32(gn64), dev), grad_dtype=torch.bfloat16)
    want = [gq_p.double() + gq_n.double(), gd_p.double(), gd_n.double()]
    for native in (False, True):
        for name, got, w in zip(("q", "d_pos", "d_neg"), steps[native][5], want):
            w = w.cpu().numpy()
            lim = R.ulp16(w, torch.bfloat16)
            if name == "q":      # the sum of two bf16 gradients, added by autograd in bf16: each part's ulp and the sum's rounding
                lim = lim + R.ulp16(gq_p.double().cpu().numpy(), torch.bfloat16) + R.ulp16(gq_n.double().cpu().numpy(), torch.bfloat16)
            err = np.abs(got.double().cpu().numpy() - w)
            print(f"step native={native} grad {name}: worst {np.max(err / lim):.2f} of the bound")
            assert np.all(err <= lim), (native, name)
