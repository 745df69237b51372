"""GPU tests of the native in-batch negatives (csrc/inbatch_loss.hip through matchmaker_amd/inbatch.py).

Yardstick: the float64 restatement (tests/inbatch_reference.py) on the exactly widened inputs.  Per case e_ref = the error of the
module's eager formula in fp32 on the CPU over the same widened inputs (tests/test_inbatch_cpu.py holds that formula to the
reference's classes).  Loss and score_diff: within 4 e_ref + 4 fp32 ulps of the value.  For the dot entry score_diff is held to
that bound against the restatement evaluated on the entry's OWN fp32 score matrices (return_scores=True; e_ref = the eager
formula on the CPU over those same matrices), and the matrices themselves are held to the fp32 dot bound E 2^-24 sum |q_k d_k| of
Q D^T: score_diff is a mean of differences that cancel, so measured against the exact dots it would ask for digits that no fp32
S holds, while on a given S every sum is float64 and the statistic is exact to one rounding.  accuracy
and teacher accuracy: exact, as counts over 2 M; sp is drawn so that no compared pair is closer than the fp32 dot bound E 2^-24 sum |q_k d_k|.  Gradients, per element: within
4 e_ref_g + 4 * 2^-24 * max |g64| (e_ref_g = the eager gradient's largest error for that tensor), plus one 16-bit ulp of the
element for 16-bit tensors.

Shapes: B in {1, 2, 3, 16, 17, 33, 65, 130} (one tile, a partial tile, the tile edge 32 / 33, more than one row tile, more than one
workgroup of four column tiles) x E in {8, 72, 768} (one partial k step, an odd number of 8-element chunks, the BERT width).
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from matchmaker_amd import _lib, inbatch, losses, ops
from tests import inbatch_reference as IR, losses_reference as R, poison, util
from tests.test_losses_gpu import assert_list_conditions

pytestmark = pytest.mark.gpu

BS = (1, 2, 3, 16, 17, 33, 65, 130)
ES = (8, 72, 768)
DT16 = (torch.float16, torch.bfloat16)
# name: (kind of tests/losses_reference.py, family, teacher)
KINDS = {"margin_mse": ("pair", True), "ranknet": ("pair", False), "mse_ranknet": ("pair", True)}      # mse_ranknet: gpos != -gneg
LIST_KINDS = {k: ("list", True) for k in R.LIST_KINDS}
CLASS = {"ranknet": losses.RankNetLoss, "margin_mse": losses.MSMarginLoss, "mse_ranknet": losses.MSERanknetTeacher,
         "listnet": losses.ListNetLoss, "kldiv": losses.KLDivTeacherList, "smooth_mrr": losses.SmoothMRRLoss,
         "lambda_ndcg2": lambda: losses.LambdaLoss("ndcgLoss2_scheme"),
         "lambda_ndcg2_teacher": lambda: losses.LambdaLossTeacher("ndcgLoss2_scheme")}
VEC = ("sp", "Q", "Dp", "Dn")


def seed_of(*key):
    return zlib.crc32("|".join(map(str, key)).encode())


def widen(x32, dtype):
    return x32 if dtype == torch.float32 else torch.from_numpy(x32).to(dtype).to(torch.float32).numpy()


def dev_t(x, dev, dtype=torch.float32):
    return None if x is None else torch.from_numpy(np.array(x)).to(dev).to(dtype)


def bits32(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def module(kind, native=True):
    family = (KINDS.get(kind) or LIST_KINDS[kind])[0]
    return inbatch.InBatchNegatives(CLASS[kind](), family == "list", native=native)


def draw(kind, B, E, dtype, salt):
    family, teacher = KINDS.get(kind) or LIST_KINDS[kind]
    rng = np.random.default_rng(seed_of("inbatch", kind, B, E, salt))
    f = np.float32
    d = {k: widen(f(rng.standard_normal((B, E)) / E ** 0.25), dtype) for k in ("Q", "Dp", "Dn")}      # dots ~ N(0, 1)
    d["Tp"] = f(3 * rng.standard_normal((B, B))) if teacher else None
    d["Tn"] = f(3 * rng.standard_normal((B, B))) if teacher else None
    for _ in range(50 if kind == "lambda_ndcg2_teacher" else 0):
        # among the softmax values of the teacher lists some always lie near the 0.001 threshold: those scores are moved by 0.25
        T = np.concatenate([d["Tp"], d["Tn"]], 1)
        near = np.abs(R.teacher_labels(T)[1].astype(np.float64) - 0.001) <= 2e-5
        if not near.any():
            break
        T[near] += f(0.25)
        d["Tp"], d["Tn"] = np.ascontiguousarray(T[:, :B]), np.ascontiguousarray(T[:, B:])
    Sp, Sn = IR.f64(d["Q"]) @ IR.f64(d["Dp"]).T, IR.f64(d["Q"]) @ IR.f64(d["Dn"]).T
    bp, bn = IR.dot_bound(d["Q"], d["Dp"]), IR.dot_bound(d["Q"], d["Dn"])
    off = IR.off_mask(B)
    sp = np.zeros(B, dtype=f)
    for i in range(B):      # sp_i is redrawn until no compared pair of its row is closer than the fp32 dot bound
        for _ in range(200):
            v = float(widen(f([2 * rng.standard_normal()]), dtype)[0])
            if np.all(np.abs(v - Sp[i])[off[i]] > bp[i][off[i]]) and np.all(np.abs(v - Sn[i])[off[i]] > bn[i][off[i]]):
                break
        else:
            raise AssertionError("no sp_i clear of the dot bound in 200 draws")
        sp[i] = v
    d["sp"] = sp
    return family, d, Sp, Sn


@functools.lru_cache(maxsize=None)
def case(kind, B, E, dtype=torch.float32):
    """inputs, float64 reference and the eager fp32 CPU result, computed once and never modified"""
    for salt in range(20):      # the first seed whose INPUTS meet the list kinds' conditions (no device result is involved)
        family, d, Sp, Sn = draw(kind, B, E, dtype, salt)
        if family == "pair":
            break
        try:
            assert_list_conditions(kind, np.float32(np.concatenate([Sp, Sn], 1)), np.concatenate([d["Tp"], d["Tn"]], 1))
            break
        except AssertionError:
            if salt == 19:
                raise
    ref64 = IR.from_vectors(family, kind, d["sp"], d["Q"], d["Dp"], d["Dn"], d["Tp"], d["Tn"])
    leaves = {k: torch.from_numpy(d[k]).requires_grad_() for k in VEC}
    T = [None if d[k] is None else torch.from_numpy(d[k]) for k in ("Tp", "Tn")]
    ref32 = {"g_" + k: np.zeros_like(d[k]) for k in VEC}
    if B > 1 or family == "list":
        loss, stats = module(kind, native=False)(leaves["sp"], leaves["Q"], leaves["Dp"], leaves["Dn"], *T)
        loss.backward()
        ref32.update({"g_" + k: t.grad.numpy() for k, t in leaves.items() if t.grad is not None})
        ref32.update(loss=loss.item(), score_diff=stats["score_diff"].item())
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return family, d, ref64, ref32


def check(label, got, ref32, ref64):
    """|got - ref64| <= 4 e_ref + 4 fp32 ulps of |ref64|; the figures are printed before the assertion"""
    err, e_ref, ulp = abs(float(got) - ref64), abs(float(ref32) - ref64), R.ulp32(abs(ref64))
    print(f"{label}: err {err:.3e} ({err / ulp:.2f} ulp) e_ref {e_ref:.3e} bound {4 * e_ref + 4 * ulp:.3e}")
    assert err <= 4 * e_ref + 4 * ulp, label


def eager_on_scores(kind, sp, Sp, Sn, Tp, Tn, dtype=torch.float32):
    """the module's eager formula in fp32 on the CPU over given score matrices: (loss, score_diff, g_sp, g_Sp, g_Sn)"""
    leaves = [torch.from_numpy(np.array(t, dtype=np.float32)).requires_grad_() for t in (sp, Sp, Sn)]
    T = [None if t is None else torch.from_numpy(np.array(t)) for t in (Tp, Tn)]
    loss, stats = module(kind, native=False).forward_scores(*leaves, *T)
    loss.backward()
    return [loss.item(), stats["score_diff"].item()] + [np.zeros(t.shape, np.float32) if t.grad is None else t.grad.numpy() for t in leaves]


def check_grad(label, got, ref32, ref64, dtype):
    got, ref32, ref64 = R.f64(got.float().cpu().numpy()), R.f64(ref32), R.f64(ref64)
    e_ref = np.abs(ref32 - ref64).max() if ref64.size else 0.0
    lim = 4 * e_ref + 4 * 2.0 ** -24 * (np.abs(ref64).max() if ref64.size else 0.0)
    lim = lim + (R.ulp16(ref64, dtype) if dtype != torch.float32 else 0.0)
    err = np.abs(got - ref64)
    print(f"{label}: worst {np.max(err / np.maximum(lim, 1e-300)) if err.size else 0:.2f} of the bound, e_ref {e_ref:.3e}")
    assert np.all(err <= lim), label


def call(kind, B, E, dtype, dev, **kw):
    family, d, ref64, ref32 = case(kind, B, E, dtype)
    args = [dev_t(d[k], dev, dtype) for k in ("Q", "Dp", "Dn", "sp")] + [dev_t(d["Tp"], dev), dev_t(d["Tn"], dev)]
    return inbatch.inbatch_dot_loss(*args, family, kind, **kw), args, (family, d, ref64, ref32)


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
def _accuracy(kind, B, E, dtype):
    dev = util.require_gpu()
    (loss, stats, gQ, gDp, gDn, gsp, Sp, Sn), args, (family, d, ref64, ref32) = call(kind, B, E, dtype, dev, return_scores=True)
    Sp, Sn = Sp.cpu().numpy(), Sn.cpu().numpy()
    assert Sp.dtype == np.float32 and Sp.shape == Sn.shape == (B, B)
    for name, S, D in (("Sp", Sp, d["Dp"]), ("Sn", Sn, d["Dn"])):      # the entry's own scores against the exact dots
        assert np.all(np.abs(R.f64(S) - ref64[name]) <= IR.dot_bound(d["Q"], D)), name + " within the fp32 dot bound"
    assert loss.shape == () and loss.dtype == stats.dtype == torch.float32 and stats.shape == (3,)
    assert gQ.dtype == gDp.dtype == gDn.dtype == gsp.dtype == dtype and gQ.shape == gDp.shape == gDn.shape == (B, E) and gsp.shape == (B,)
    tag = f"{kind} B={B} E={E} {dtype}"
    st = stats.cpu().numpy()
    if B == 1:
        assert np.isnan(st[0]) and np.isnan(st[1]), "means of empty sets"
    if B == 1 and family == "pair":
        assert np.isnan(loss.item()) and np.isnan(st).all()
        for g in (gQ, gDp, gDn, gsp):
            assert not poison.bits(g).any(), "B = 1: gradients 0"
        return
    check(tag + " loss", loss.item(), ref32["loss"], ref64["loss"])
    if B > 1:
        on_own = IR.from_scores("pair", "ranknet", d["sp"], Sp, Sn)["score_diff"]      # (the statistic does not depend on the kind)
        check(tag + " score_diff", st[1], eager_on_scores(kind, d["sp"], Sp, Sn, d["Tp"], d["Tn"])[1], on_own)
        n, M2, t = IR.counts(d["sp"], ref64["Sp"], ref64["Sn"], d["Tp"], d["Tn"])
        assert bits32(st[0]) == bits32(n / M2), "accuracy is exact"
        if family == "pair" and d["Tp"] is not None:
            assert bits32(st[2]) == bits32(t / M2), "teacher accuracy is exact"
        else:
            assert np.isnan(st[2])
    for k, g in zip(VEC, (gsp, gQ, gDp, gDn)):
        check_grad(f"{tag} g_{k}", g, ref32["g_" + k], ref64["g_" + k], dtype)
    if family == "list":
        assert not poison.bits(gsp).any(), "the list family does not use sp"


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_pair_accuracy_fp32(kind, B, E):
    _accuracy(kind, B, E, torch.float32)


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("B", (3, 33))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_pair_accuracy_16bit(kind, B, E, dtype):
    _accuracy(kind, B, E, dtype)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("B", (1, 3, 33))
@pytest.mark.parametrize("kind", sorted(LIST_KINDS))
def test_list_accuracy_fp32(kind, B, E):
    _accuracy(kind, B, E, torch.float32)


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("B", (3, 33))
@pytest.mark.parametrize("kind", sorted(LIST_KINDS))
def test_list_accuracy_16bit(kind, B, E, dtype):
    _accuracy(kind, B, E, dtype)


SELECT_KINDS = ("margin_mse", "mse_ranknet", "ranknet", "kldiv", "listnet", "lambda_ndcg2_teacher")


@pytest.mark.parametrize("dtype", (torch.float32,) + DT16)
@pytest.mark.parametrize("kind", SELECT_KINDS)
def test_select_entry_accuracy(kind, dtype):
    """the select entry on given score matrices (the exact dots rounded to `dtype`): loss and score_diff at 4 e_ref + 4 ulps of
    the value, the counts exact, grad_sp / grad_Sp / grad_Sn at the gradient bound, all against the restatement on those matrices"""
    dev = util.require_gpu()
    B = 33
    family, d, r, _ = case(kind, B, 72, dtype)
    sp, Sp, Sn = d["sp"], widen(np.float32(r["Sp"]), dtype), widen(np.float32(r["Sn"]), dtype)
    ref64 = IR.from_scores(family, kind, sp, Sp, Sn, d["Tp"], d["Tn"])
    e = eager_on_scores(kind, sp, Sp, Sn, d["Tp"], d["Tn"])
    loss, stats, gsp, gSp, gSn = inbatch.inbatch_select_loss(dev_t(sp, dev, dtype), dev_t(Sp, dev, dtype), dev_t(Sn, dev, dtype),
                                                             dev_t(d["Tp"], dev), dev_t(d["Tn"], dev), family, kind)
    assert gsp.dtype == gSp.dtype == gSn.dtype == dtype and gSp.shape == gSn.shape == (B, B)
    tag = f"select {kind} {dtype}"
    check(tag + " loss", loss.item(), e[0], ref64["loss"])
    check(tag + " score_diff", stats[1].item(), e[1], ref64["score_diff"])
    n, M2, t = IR.counts(sp, Sp, Sn, d["Tp"], d["Tn"])
    assert bits32(stats[0].item()) == bits32(n / M2)
    assert bits32(stats[2].item()) == bits32(t / M2) if family == "pair" and d["Tp"] is not None else np.isnan(stats[2].item())
    for name, got, e32 in (("g_sp", gsp, e[2]), ("g_Sp", gSp, e[3]), ("g_Sn", gSn, e[4])):
        check_grad(f"{tag} {name}", got, e32, ref64[name], dtype)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def exact_inputs(B, E, seed=1):
    """vectors of small integers / 4, integer sp and teachers: every product, sum and Margin-MSE term is exact in fp32 / float64"""
    rng = np.random.default_rng(seed_of("exact", B, E, seed))
    f = np.float32
    Q, Dp, Dn = (f(rng.integers(-3, 4, (B, E))) / f(4) for _ in range(3))
    sp, Tp, Tn = f(rng.integers(-4, 5, B)), f(rng.integers(-6, 7, (B, B))), f(rng.integers(-6, 7, (B, B)))
    return Q, Dp, Dn, sp, Tp, Tn


@pytest.mark.parametrize("B", BS)
def test_exact_inputs_give_the_float64_loss_rounded_once(B):
    dev = util.require_gpu()
    E = 72
    Q, Dp, Dn, sp, Tp, Tn = exact_inputs(B, E)
    if B > 1:      # a planted tie: sp_0 == Sp_01 exactly
        sp[0] = np.float32(IR.f64(Q[0]) @ IR.f64(Dp[1]))
    r = IR.from_vectors("pair", "margin_mse", sp, Q, Dp, Dn, Tp, Tn)
    out = inbatch.inbatch_dot_loss(*[dev_t(t, dev) for t in (Q, Dp, Dn, sp, Tp, Tn)], "pair", "margin_mse", return_scores=True)
    loss, stats, gQ, gDp, gDn, gsp, Sp, Sn = out
    assert np.array_equal(Sp.cpu().numpy(), np.float32(r["Sp"])) and np.array_equal(Sn.cpu().numpy(), np.float32(r["Sn"])), "Q serves both products"
    if B == 1:
        assert np.isnan(loss.item())
        return
    assert bits32(loss.item()) == bits32(r["loss"])
    n, M2, t = IR.counts(sp, r["Sp"], r["Sn"], Tp, Tn)
    assert not (sp[0] > r["Sp"][0, 1]) and bits32(stats[0].item()) == bits32(n / M2), "a tie counts as not greater"
    assert bits32(stats[1].item()) == bits32(r["score_diff"]) and bits32(stats[2].item()) == bits32(t / M2)
    sel = inbatch.inbatch_select_loss(dev_t(sp, dev), Sp, Sn, dev_t(Tp, dev), dev_t(Tn, dev), "pair", "margin_mse")
    assert not poison.bits(sel[3].diagonal()).any() and not poison.bits(sel[4].diagonal()).any(), "grad_S's diagonal is +0"
    if B == 2:      # M = 2: the 1 / (2 M) is a power of two, every gradient is exact
        for k, g in zip(VEC, (gsp, gQ, gDp, gDn)):
            assert np.array_equal(bits32(g.cpu().numpy()), bits32(r["g_" + k])), k
        assert np.array_equal(bits32(sel[3].cpu().numpy()), bits32(r["g_Sp"])) and np.array_equal(bits32(sel[4].cpu().numpy()), bits32(r["g_Sn"]))


# ---- semantics --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("margin_mse", "kldiv"))
def test_diagonal_is_excluded_for_pairs_and_included_for_lists(kind):
    dev = util.require_gpu()
    family, d, ref64, _ = case(kind, 17, 72)
    sp, Tp, Tn = dev_t(d["sp"], dev), dev_t(d["Tp"], dev), dev_t(d["Tn"], dev)
    Sp, Sn = dev_t(np.float32(ref64["Sp"]), dev), dev_t(np.float32(ref64["Sn"]), dev)
    a = inbatch.inbatch_select_loss(sp, Sp, Sn, Tp, Tn, family, kind)
    Sp2, Sn2 = Sp.clone(), Sn.clone()
    Sp2.diagonal().add_(1.5)
    Sn2.diagonal().sub_(0.75)
    b = inbatch.inbatch_select_loss(sp, Sp2, Sn2, Tp, Tn, family, kind)
    if family == "pair":
        poison.assert_same_bits(a, b, "the diagonal takes no part")
    else:
        assert a[0].item() != b[0].item() and torch.equal(poison.bits(a[1]), poison.bits(b[1])), "loss moves, statistics do not"
        assert a[3].diagonal().abs().min() > 0, "the diagonal has a gradient"


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16))
@pytest.mark.parametrize("kind,B", [("margin_mse", 33), ("ranknet", 130), ("mse_ranknet", 17), ("kldiv", 33), ("lambda_ndcg2_teacher", 3)])
def test_dot_entry_equals_select_entry_on_its_own_scores_and_loss_only_call(kind, B, dtype):
    dev = util.require_gpu()
    out, args, (family, d, _, _) = call(kind, B, 72, dtype, dev, return_scores=True)
    loss, stats, gQ, gDp, gDn, gsp, Sp, Sn = out
    assert Sp.dtype == torch.float32
    sel = inbatch.inbatch_select_loss(args[3].float(), Sp, Sn, args[4], args[5], family, kind)
    assert torch.equal(poison.bits(sel[0]), poison.bits(loss)) and torch.equal(poison.bits(sel[1]), poison.bits(stats))
    if dtype == torch.float32:
        assert torch.equal(poison.bits(sel[2]), poison.bits(gsp))
        sp_np, Sp_np, Sn_np = (t.cpu().numpy() for t in (args[3], Sp, Sn))      # the select entry's matrix gradients on these scores
        r = IR.from_scores(family, kind, sp_np, Sp_np, Sn_np, d["Tp"], d["Tn"])
        e = eager_on_scores(kind, sp_np, Sp_np, Sn_np, d["Tp"], d["Tn"])
        check_grad(f"{kind} B={B} select g_Sp", sel[3], e[3], r["g_Sp"], dtype)
        check_grad(f"{kind} B={B} select g_Sn", sel[4], e[4], r["g_Sn"], dtype)
    only = inbatch.inbatch_dot_loss(*args, family, kind, need_grad=False)
    assert only[2:] == (None, None, None, None)
    assert torch.equal(poison.bits(only[0]), poison.bits(loss)) and torch.equal(poison.bits(only[1]), poison.bits(stats))


@pytest.mark.parametrize("kind", ("margin_mse", "kldiv"))
def test_colbert_route_through_forward_scores(kind):
    """32 x 32 all-pairs MaxSim matrices -> forward_scores: the loss and statistics of the restatement, backward = the select
    entry's saved gradients"""
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(11)
    B, Qn, Dn_, E = 32, 8, 24, 32
    q = (torch.randn(B, Qn, E, generator=g) / E ** 0.5).to(dev).to(torch.float16)
    dp, dn = ((torch.randn(B, Dn_, E, generator=g) / E ** 0.5).to(dev).to(torch.float16) for _ in range(2))
    Sp = ops.maxsim_inbatch(q, None, dp, None).requires_grad_()
    Sn = ops.maxsim_inbatch(q, None, dn, None).requires_grad_()
    sp = Sp.detach().diagonal().clone().requires_grad_()
    Tp, Tn = (3 * torch.randn(B, B, generator=g)).to(dev), (3 * torch.randn(B, B, generator=g)).to(dev)
    mod = module(kind)
    assert mod.scores_route(sp, Sp, Sn, Tp, Tn)
    loss, stats = mod.forward_scores(sp, Sp, Sn, Tp, Tn)
    assert "SelectLoss" in type(loss.grad_fn).__name__
    (loss * 2.0).backward()
    family = mod.family_kind[0]
    saved = inbatch.inbatch_select_loss(sp, Sp, Sn, Tp, Tn, *mod.family_kind)
    for t, s in zip((sp, Sp, Sn), saved[2:]):
        assert torch.equal(poison.bits(t.grad), poison.bits(s * 2.0))
    r = IR.from_scores("pair" if family == inbatch.PAIR else "list", kind, *[t.detach().cpu().numpy() for t in (sp, Sp, Sn, Tp, Tn)])
    e_loss, e_stats = module(kind, native=False).forward_scores(*[t.detach().cpu() for t in (sp, Sp, Sn, Tp, Tn)])
    check(kind + " colbert loss", loss.item(), e_loss.item(), r["loss"])
    check(kind + " colbert score_diff", stats["score_diff"].item(), e_stats["score_diff"].item(), r["score_diff"])
    assert (stats["teacher_accuracy"] is None) == (family == inbatch.LIST)


# ---- module, autograd, torch ops ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("margin_mse", "ranknet", "listnet"))
def test_module_backward_is_the_saved_gradient_times_grad_output(kind):
    dev = util.require_gpu()
    import matchmaker_amd.torch_ops  # noqa: F401
    (loss0, stats0, gQ, gDp, gDn, gsp), args, (family, d, _, _) = call(kind, 17, 72, torch.float32, dev)
    Q, Dp, Dn, sp, Tp, Tn = args
    before = [poison.bits(t).clone() for t in args if t is not None]
    leaves = [t.clone().requires_grad_() for t in (sp, Q, Dp, Dn)]
    mod = module(kind)
    assert mod.dot_route(*leaves, Tp, Tn)
    loss, stats = mod(*leaves, Tp, Tn)
    assert "DotLoss" in type(loss.grad_fn).__name__ and torch.equal(poison.bits(loss), poison.bits(loss0))
    assert torch.equal(poison.bits(stats["accuracy"]), poison.bits(stats0[0])) and not stats["accuracy"].requires_grad
    (loss * 1024.0).backward()
    for t, s in zip(leaves, (gsp, gQ, gDp, gDn)):
        assert torch.equal(poison.bits(t.grad), poison.bits(s * 1024.0)), "backward = 1024 x the saved gradient, exactly"
    for t, b in zip([t for t in args if t is not None], before):
        assert torch.equal(poison.bits(t), b), "inputs are bit-unchanged"
    with torch.no_grad():
        assert torch.equal(poison.bits(mod(sp, Q, Dp, Dn, Tp, Tn)[0]), poison.bits(loss0))
    leaves = [t.clone().requires_grad_() for t in (Q, Dp, Dn, sp)]
    out = torch.ops.mm_native.inbatch_dot_loss(*leaves, Tp, Tn, *mod.family_kind)
    out[0].backward()
    for t, s in zip(leaves, (gQ, gDp, gDn, gsp)):
        assert torch.equal(poison.bits(t.grad), poison.bits(s))
    eager = module(kind, native=False)
    leaves = [t.clone().requires_grad_() for t in (sp, Q, Dp, Dn)]
    e_loss, _ = eager(*leaves, Tp, Tn)
    assert "DotLoss" not in type(e_loss.grad_fn).__name__ and abs(e_loss.item() - loss0.item()) <= 1e-4 * abs(loss0.item())


@pytest.mark.parametrize("dtype", DT16)
def test_backward_under_a_large_loss_scale_is_formed_in_fp32(dtype):
    """grad_output = 2^17 (a GradScaler's scale times lambda) does not fit fp16; saved gradient x grad_output does (RankNet:
    |d loss / d S| <= 1 / (2 M), so every product here is below 2^13)"""
    dev = util.require_gpu()
    import matchmaker_amd.torch_ops  # noqa: F401
    (_, _, gQ, gDp, gDn, gsp), args, (family, d, _, _) = call("ranknet", 33, 72, dtype, dev)
    Q, Dp, Dn, sp, Tp, Tn = args
    scale = torch.tensor(2.0 ** 17, device=dev)
    want = [(t.float() * scale).to(dtype) for t in (gsp, gQ, gDp, gDn)]
    assert all(torch.isfinite(w).all() for w in want) and gQ.abs().max() > 0
    mod = module("ranknet")
    for route in ("module", "op"):
        leaves = [t.clone().requires_grad_() for t in (sp, Q, Dp, Dn)]
        if route == "module":
            loss = mod(*leaves, Tp, Tn)[0]
        else:
            loss = torch.ops.mm_native.inbatch_dot_loss(leaves[1], leaves[2], leaves[3], leaves[0], Tp, Tn, *mod.family_kind)[0]
        (loss * scale).backward()
        for t, w in zip(leaves, want):
            assert torch.equal(poison.bits(t.grad), poison.bits(w)), route
    Sp, Sn = (Q.float() @ Dp.float().T).to(dtype), (Q.float() @ Dn.float().T).to(dtype)
    leaves = [t.clone().requires_grad_() for t in (sp, Sp, Sn)]
    saved = inbatch.inbatch_select_loss(*leaves, Tp, Tn, *mod.family_kind)[2:]
    (mod.forward_scores(*leaves, Tp, Tn)[0] * scale).backward()
    for t, g in zip(leaves, saved):
        assert torch.isfinite(t.grad).all() and torch.equal(poison.bits(t.grad), poison.bits((g.float() * scale).to(dtype)))


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16))
def test_vectors_at_an_unaligned_address_give_the_same_bits(dtype):
    """a contiguous view whose storage offset is no multiple of 16 bytes: the wrapper copies it; the C entry refuses it"""
    dev = util.require_gpu()
    out, args, (family, d, _, _) = call("margin_mse", 17, 72, dtype, dev)
    shifted = []
    for t in args[:3]:
        buf = torch.empty(t.numel() + 1, dtype=dtype, device=dev)
        buf[1:].copy_(t.reshape(-1))
        shifted.append(buf[1:].view(t.shape))
        assert shifted[-1].is_contiguous() and shifted[-1].data_ptr() % 16 != 0
    poison.assert_same_bits(out, inbatch.inbatch_dot_loss(*shifted, *args[3:], family, "margin_mse"), "unaligned vectors")
    leaves = [t.clone().requires_grad_() for t in [args[3]] + shifted]
    mod = module("margin_mse")
    assert mod.dot_route(*leaves, args[4], args[5])
    assert torch.equal(poison.bits(mod(*leaves, args[4], args[5])[0]), poison.bits(out[0]))
    L = _lib.lib()
    p = [t.data_ptr() for t in out]
    rc = L.mm_inbatch_dot_loss_fwd(shifted[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), ops._DT[dtype], args[3].data_ptr(),
                                   ops._DT[dtype], args[4].data_ptr(), args[5].data_ptr(), 17, 72, inbatch.PAIR, _lib.PAIR_MARGIN_MSE,
                                   p[0], p[1], p[2], p[3], p[4], p[5], None, 0, None)
    assert rc == _lib.MM_EINVAL and b"aligned" in L.mm_last_error()


def test_teacher_that_requires_grad_and_refused_shapes_stay_eager_on_the_device():
    dev = util.require_gpu()
    (_, _, _, _, _, _), args, _ = call("margin_mse", 17, 72, torch.float32, dev)
    Q, Dp, Dn, sp, Tp, Tn = args
    mod = module("margin_mse")
    loss, _ = mod(sp, Q.clone().requires_grad_(), Dp, Dn, Tp.clone().requires_grad_(), Tn)
    assert "DotLoss" not in type(loss.grad_fn).__name__
    h = torch.float16
    loss, _ = mod(sp, Q[:, :12].to(h).requires_grad_(), Dp[:, :12].to(h), Dn[:, :12].to(h), Tp, Tn)      # rows of 24 bytes
    assert "DotLoss" not in type(loss.grad_fn).__name__ and torch.isfinite(loss)
    with pytest.raises(_lib.NativeError) as e:
        inbatch.inbatch_dot_loss(Q[:, :12].to(h).contiguous(), Dp[:, :12].to(h).contiguous(), Dn[:, :12].to(h).contiguous(), sp, Tp, Tn, "pair", "margin_mse")
    assert e.value.code == _lib.MM_EUNSUPPORTED
    empty = inbatch.inbatch_dot_loss(Q[:0], Dp[:0], Dn[:0], sp[:0], None, None, "pair", "ranknet")
    assert np.isnan(empty[0].item()) and empty[2].shape == (0, 72)


# ---- determinism and capture --------------------------------------------------------------------------------------------------------
CAPTURE = [("margin_mse", 33, 72, torch.float16), ("ranknet", 130, 8, torch.float32), ("kldiv", 33, 72, torch.float32),
           ("lambda_ndcg2_teacher", 17, 768, torch.bfloat16)]


@pytest.mark.parametrize("kind,B,E,dtype", CAPTURE)
def test_two_calls_and_a_captured_replay_on_fresh_values_give_the_same_bits(kind, B, E, dtype):
    dev = util.require_gpu()
    first, args, (family, d, _, _) = call(kind, B, E, dtype, dev)
    fn = lambda: inbatch.inbatch_dot_loss(*args, family, kind)  # noqa: E731
    poison.assert_same_bits(first, fn(), "two calls")
    fresh = [t.flip(0).contiguous() for t in args[:4]]      # other values of the same shapes
    assert not torch.equal(fresh[0], args[0])
    static = [t.clone() if t is not None else None for t in args]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up off the default stream, as torch.cuda.graph asks
        inbatch.inbatch_dot_loss(*static, family, kind)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # one stream, one linear chain of launches: no parallel branches
        out = inbatch.inbatch_dot_loss(*static, family, kind)
    for s, t in zip(static, fresh):
        s.copy_(t)
    want = inbatch.inbatch_dot_loss(*static, family, kind)
    for t in out:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    poison.assert_same_bits(want, out, "captured replay")


# ---- poisoned memory ----------------------------------------------------------------------------------------------------------------
POISON = [("dot", "margin_mse", 33, 72, torch.float16), ("dot", "mse_ranknet", 130, 8, torch.float32), ("dot", "kldiv", 33, 72, torch.float32),
          ("dot", "lambda_ndcg2", 17, 72, torch.bfloat16), ("select", "margin_mse", 65, 8, torch.float32), ("select", "listnet", 3, 8, torch.float16),
          ("dot", "ranknet", 1, 8, torch.float32)]


@pytest.mark.parametrize("entry,kind,B,E,dtype", POISON)
def test_every_output_is_written_whatever_the_memory_held(entry, kind, B, E, dtype):
    dev = util.require_gpu()
    family, d, ref64, _ = case(kind, B, E, dtype)
    vec = [dev_t(d[k], dev, dtype) for k in ("Q", "Dp", "Dn", "sp")]
    T = [dev_t(d["Tp"], dev), dev_t(d["Tn"], dev)]
    if entry == "dot":
        inputs = vec + T
        fn = lambda: inbatch.inbatch_dot_loss(*inputs, family, kind)  # noqa: E731
    else:
        inputs = [vec[3], dev_t(np.float32(ref64["Sp"]), dev, dtype), dev_t(np.float32(ref64["Sn"]), dev, dtype)] + T
        fn = lambda: inbatch.inbatch_select_loss(*inputs, family, kind)  # noqa: E731
    before = [poison.bits(t).clone() for t in inputs if t is not None]
    outs = []
    for p in poison.POISONS:
        out, arena = poison.run(fn, p, module=inbatch, label=f"{entry} {kind} {B} {E}")
        assert len(arena.allocations) == (7 if entry == "dot" else 6), "outputs and the workspace came from the arena"
        outs.append(out)
    poison.assert_same_bits(outs[0], outs[1], f"{entry} {kind} {B} {E}")
    poison.assert_same_bits(outs[0], fn(), "against an unpoisoned call")
    for t, b in zip([t for t in inputs if t is not None], before):
        assert torch.equal(poison.bits(t), b), "inputs are untouched"
