"""CPU tests of the native in-batch negatives (matchmaker_amd/inbatch.py over csrc/inbatch_loss.hip): the float64 restatement
and the module's eager formula against the goldens recorded from the real reference classes, autograd of the eager formula
against finite differences, the class -> (family, kind) map, the C boundary and its refusals, the fake implementations of the
torch ops and the routes that stay eager."""
import re
import sys
import warnings

import numpy as np
import pytest
import torch

from matchmaker_amd import _lib, inbatch, losses
from tests import abi, inbatch_reference as IR, losses_reference as R, util

sys.path.insert(0, util.GOLDEN)
from gen_golden_inbatch import CASES  # noqa: E402  (the case table only: names, kinds, shapes)

GOLD = util.load("inbatch_cases.npz")
CLASS = {"ranknet": losses.RankNetLoss, "margin_mse": losses.MSMarginLoss, "ranknet_teacher": losses.RankNetTeacher,
         "kldiv": losses.KLDivTeacherList, "listnet": losses.ListNetLoss,
         "lambda_ndcg2_teacher": lambda: losses.LambdaLossTeacher("ndcgLoss2_scheme")}
VEC = ("sp", "Q", "Dp", "Dn")


def case(name):
    return {k[len(name) + 1:]: v for k, v in GOLD.items() if k.startswith(name + ".")}


def close32(got, want, ulps=64):
    """fp32-class agreement: within `ulps` fp32 ulps of the largest magnitude (sums of <= 2 * 56 fp32 terms of dots of <= 16)"""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() <= ulps * R.ulp32(max(np.abs(want).max(), 1e-30))


def run_module(name, dtype=torch.float32):
    kind, family, teacher, B, E = CASES[name]
    d = case(name)
    mod = inbatch.InBatchNegatives(CLASS[kind](), family == "list", native=True)      # CPU tensors: the eager route all the same
    leaves = {k: torch.from_numpy(d[k]).to(dtype).requires_grad_() for k in VEC}
    T = [torch.from_numpy(d[k]).to(dtype) if teacher else None for k in ("Tp", "Tn")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss, stats = mod(leaves["sp"], leaves["Q"], leaves["Dp"], leaves["Dn"], *T)
    return d, leaves, T, loss, stats, mod


# ---- 1. restatement and eager formula against the goldens ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_goldens(name):
    kind, family, teacher, B, E = CASES[name]
    d = case(name)
    r = IR.from_vectors(family, kind, d["sp"], d["Q"], d["Dp"], d["Dn"], d.get("Tp"), d.get("Tn"))
    assert close32(d["loss"], r["loss"]) and close32(d["score_diff"], r["score_diff"])
    n, M2, t = IR.counts(d["sp"], r["Sp"], r["Sn"], d.get("Tp"), d.get("Tn"))
    assert M2 == 2 * B * (B - 1) and round(float(d["accuracy"]) * M2) == n
    if family == "pair" and teacher:
        assert round(float(d["teacher_accuracy"]) * M2) == t
    else:
        assert r["teacher_accuracy"] is None and "teacher_accuracy" not in d
    for k in VEC:
        assert close32(d["g_" + k], r["g_" + k]), k
    assert not np.diagonal(r["g_Sp"]).any() or family == "list"
    if family == "list":
        assert not r["g_sp"].any() and not d["g_sp"].any() and np.diagonal(r["g_Sp"]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_eager_formula_matches_the_goldens(name):
    d, leaves, T, loss, stats, mod = run_module(name)
    loss.backward()
    assert close32(loss.detach().numpy(), d["loss"], ulps=8)
    assert stats["accuracy"] == float(d["accuracy"]) and close32(stats["score_diff"].numpy(), d["score_diff"], ulps=8)
    assert not stats["accuracy"].requires_grad and not stats["score_diff"].requires_grad
    if "teacher_accuracy" in d:
        assert stats["teacher_accuracy"] == float(d["teacher_accuracy"])
    else:
        assert stats["teacher_accuracy"] is None
    for k in VEC:
        got = leaves[k].grad.numpy() if leaves[k].grad is not None else np.zeros_like(d[k])
        assert close32(got, d["g_" + k], ulps=8), k


def test_forward_scores_is_the_same_formula_on_the_matrices():
    d, leaves, T, loss, stats, mod = run_module("margin_mse_8x16")
    Sp, Sn = leaves["Q"].detach() @ leaves["Dp"].detach().T, leaves["Q"].detach() @ leaves["Dn"].detach().T
    loss2, stats2 = mod.forward_scores(leaves["sp"].detach(), Sp, Sn, *T)
    assert torch.equal(loss2, loss.detach()) and all(torch.equal(stats2[k], stats[k]) for k in stats)


def test_query_of_the_positive_pair_serves_both_products():
    """Sn = Q Dn^T with the SAME query vectors (train.py:440 uses query_vecs_pos for both)"""
    d = case("margin_mse_3x8")
    r = IR.from_vectors("pair", "margin_mse", d["sp"], d["Q"], d["Dp"], d["Dn"], d["Tp"], d["Tn"])
    assert np.array_equal(r["Sn"], d["Q"].astype(np.float64) @ d["Dn"].astype(np.float64).T)


# ---- 2. autograd of the eager formula against finite differences ------------------------------------------------------------
@pytest.mark.parametrize("name", ("margin_mse_3x8", "ranknet_7x12", "kldiv_6x16", "listnet_4x8"))
def test_eager_autograd_matches_finite_differences_in_float64(name):
    kind, family, teacher, B, E = CASES[name]
    d = case(name)
    mod = inbatch.InBatchNegatives(CLASS[kind](), family == "list")
    leaves = [torch.from_numpy(d[k]).double().requires_grad_() for k in VEC]
    T = [torch.from_numpy(d[k]).double() if teacher else None for k in ("Tp", "Tn")]
    assert torch.autograd.gradcheck(lambda sp, Q, Dp, Dn: mod(sp, Q, Dp, Dn, *T)[0], leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


# ---- 3. class -> (family, kind) ------------------------------------------------------------------------------------------------
def test_class_to_family_and_kind():
    P, Ls = inbatch.PAIR, inbatch.LIST
    want = {losses.RankNetLoss: (P, _lib.PAIR_RANKNET), losses.MSMarginLoss: (P, _lib.PAIR_MARGIN_MSE),
            losses.MSETeacherPointwise: (P, _lib.PAIR_MSE_POINTWISE), losses.KLDivTeacherPointwise: (P, _lib.PAIR_KLDIV_POINTWISE),
            losses.RankNetTeacher: (P, _lib.PAIR_RANKNET_TEACHER), losses.MSERanknetTeacher: (P, _lib.PAIR_MSE_RANKNET),
            losses.MarginRankingLoss1: (P, _lib.PAIR_MARGIN), losses.KLDivTeacherList: (Ls, _lib.LIST_KLDIV),
            losses.ListNetLoss: (Ls, _lib.LIST_LISTNET), losses.SmoothMRRLoss: (Ls, _lib.LIST_SMOOTH_MRR)}
    for cls, fk in want.items():
        assert inbatch.family_kind_of(cls()) == fk, cls
    assert inbatch.family_kind_of(losses.LambdaLossTeacher("ndcgLoss2_scheme")) == (Ls, _lib.LIST_LAMBDA_NDCG2_TEACHER)
    assert inbatch.family_kind_of(losses.LambdaLoss("ndcgLoss2_scheme")) == (Ls, _lib.LIST_LAMBDA_NDCG2)
    assert inbatch.family_kind_of(losses.LambdaLossTeacher("lamdbaRank_scheme")) is None
    assert inbatch.family_kind_of(torch.nn.MarginRankingLoss(margin=1)) == (P, _lib.PAIR_MARGIN)
    assert inbatch.family_kind_of(torch.nn.MarginRankingLoss(margin=0.5)) is None
    assert inbatch.family_kind_of(torch.nn.MSELoss()) is None and inbatch.family_kind_of(lambda *a: 0) is None
    # the reference's own classes go by module and class name
    for mod_name, cls_name, fk in (("matchmaker.losses.msmargin", "MSMarginLoss", (P, _lib.PAIR_MARGIN_MSE)),
                                   ("matchmaker.losses.ranknet", "RankNetLoss", (P, _lib.PAIR_RANKNET)),
                                   ("matchmaker.losses.teacher_kldiv_list", "KLDivTeacherList", (Ls, _lib.LIST_KLDIV))):
        cls = type(cls_name, (torch.nn.Module,), {"__module__": mod_name})
        assert inbatch.family_kind_of(cls()) == fk
    stranger = type("MSMarginLoss", (torch.nn.Module,), {"__module__": "somewhere.else"})
    assert inbatch.family_kind_of(stranger()) is None
    # a list loss handed over as a pair loss (or the reverse) is not a kernel case
    assert inbatch.InBatchNegatives(losses.KLDivTeacherList(), False).family_kind is None
    assert inbatch.InBatchNegatives(losses.MSMarginLoss(), True).family_kind is None
    assert inbatch.InBatchNegatives(losses.MSMarginLoss(), False).family_kind == (P, _lib.PAIR_MARGIN_MSE)


def test_native_defaults_follow_the_measured_rule():
    """True for a family only if the slowest native round beat the fastest eager round in every leg of every run"""
    assert inbatch.NATIVE_DEFAULT == {inbatch.PAIR: True, inbatch.LIST: True}
    assert inbatch.InBatchNegatives(losses.MSMarginLoss()).native is True
    assert inbatch.InBatchNegatives(losses.MSMarginLoss(), native=False).native is False
    assert inbatch.InBatchNegatives(torch.nn.MSELoss()).native is False      # a loss the kernels do not know: the eager formula


# ---- 4. symbols, header -----------------------------------------------------------------------------------------------------------
ENTRIES = ("mm_inbatch_select_loss_fwd", "mm_inbatch_dot_loss_fwd")


def test_symbols_are_bound_and_the_header_cites_what_it_replaces():
    L = abi.assert_bound(ENTRIES + ("mm_inbatch_dot_loss_workspace_bytes", "mm_inbatch_select_loss_workspace_bytes"))
    assert _lib.ABI_VERSION == 4 == L.mm_abi_version()
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for entry in ENTRIES:
        block = text[text.index(entry + " (additive: MM_ABI_VERSION unchanged)"):]
        block = block[:block.index("*/")]
        assert re.search(r"Replaces: matchmaker/train\.py:434-4\d\d", block), entry
    assert "STATED CHOICE: S stays fp32" in text
    assert (_lib.INBATCH_PAIR, _lib.INBATCH_LIST) == (0, 1) == (inbatch.PAIR, inbatch.LIST)
    res, args = _lib.SIGNATURES["mm_inbatch_dot_loss_fwd"]
    assert len(args) == 21 and res is _lib.ctypes.c_int and args[-2] is _lib.ctypes.c_size_t
    assert len(_lib.SIGNATURES["mm_inbatch_select_loss_fwd"][1]) == 17
    assert _lib.SIGNATURES["mm_inbatch_dot_loss_workspace_bytes"] == (_lib.ctypes.c_size_t, [_lib.ctypes.c_int] * 3)


def test_workspace_holds_scores_gradients_and_float64_partials():
    L = abi.assert_bound(("mm_inbatch_dot_loss_workspace_bytes",))
    for B in (1, 2, 33, 130, 1024):
        tiles = -(-2 * B // 32)
        groups = -(-tiles // 4) * -(-B // 32)
        need = 2 * (2 * B * B * 4) + groups * 4 * 8 + tiles * B * 8 + B * 4
        got = L.mm_inbatch_dot_loss_workspace_bytes(B, 768, inbatch.PAIR)
        assert need <= got <= need + 5 * 256 and got % 256 == 0, (B, need, got)
        assert got == L.mm_inbatch_dot_loss_workspace_bytes(B, 8, inbatch.LIST)
        assert L.mm_inbatch_select_loss_workspace_bytes(B, inbatch.PAIR) == got - 2 * (-(-2 * B * B * 4 // 256) * 256)


# ---- 5. refusals of the C boundary (before any launch: no device needed) ------------------------------------------------------
def test_c_abi_refusals_need_no_device():
    L = abi.assert_bound(ENTRIES)
    p = 4096      # never dereferenced: every call below is refused first
    MSE, RN, KL = _lib.PAIR_MARGIN_MSE, _lib.PAIR_RANKNET, _lib.LIST_KLDIV

    def dot(B, E, family=inbatch.PAIR, kind=MSE, dtype=_lib.MM_F16, spdt=_lib.MM_F32, Tp=p, Tn=p, loss=p, Q=p, ws=p, wsb=1 << 30):
        return L.mm_inbatch_dot_loss_fwd(Q, p, p, dtype, p, spdt, Tp, Tn, B, E, family, kind, loss, p, p, p, p, p, ws, wsb, None)

    def sel(B, family=inbatch.PAIR, kind=MSE, dtype=_lib.MM_F32, Tp=p, Tn=p, gsp=p, wsb=1 << 30):
        return L.mm_inbatch_select_loss_fwd(p, p, p, dtype, Tp, Tn, B, family, kind, p, p, gsp, p, p, p, wsb, None)

    U, I = _lib.MM_EUNSUPPORTED, _lib.MM_EINVAL
    assert dot(8, 12) == U and b"E=12" in L.mm_last_error()                     # fp16 rows of 24 bytes
    assert dot(8, 12, dtype=_lib.MM_F32, wsb=0) == _lib.MM_EWORKSPACE             # fp32 rows of 48 bytes pass the shape check
    assert dot(8, 4, dtype=_lib.MM_F32) == U and dot(8, 1032) == U and dot(8, 10, dtype=_lib.MM_F32) == U
    assert dot(1025, 64) == U and b"1025" in L.mm_last_error() and sel(1025) == U
    assert dot(513, 64, inbatch.LIST, KL) == U and b"1026" in L.mm_last_error() and sel(513, inbatch.LIST, KL) == U
    assert dot(-1, 64) == I and sel(-1) == I
    assert dot(8, 64, family=2) == I and dot(8, 64, kind=7) == I and dot(8, 64, inbatch.LIST, 5) == I and sel(8, kind=-1) == I
    assert dot(8, 64, dtype=3) == I and dot(8, 64, spdt=5) == I and sel(8, dtype=9) == I
    assert dot(8, 64, loss=None) == I and dot(8, 64, Q=None) == I and sel(8, gsp=None) == I
    assert dot(8, 64, Q=p + 8) == I and b"aligned" in L.mm_last_error()      # rows are loaded 16 bytes per lane
    assert dot(8, 64, Tn=None) == I                                             # one teacher matrix without the other
    assert dot(8, 64, Tp=None, Tn=None) == I and b"teacher" in L.mm_last_error()      # Margin-MSE has two labels
    assert dot(8, 64, kind=RN) == I and sel(8, kind=RN) == I                    # RankNet takes the label 1
    assert dot(8, 64, inbatch.LIST, KL, Tp=None, Tn=None) == I
    assert dot(8, 64, wsb=100) == _lib.MM_EWORKSPACE and dot(8, 64, ws=None) == _lib.MM_EWORKSPACE and sel(8, wsb=8) == _lib.MM_EWORKSPACE


# ---- 6. fake implementations of the torch ops ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16, torch.bfloat16))
def test_fake_shapes_and_dtypes(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import matchmaker_amd.torch_ops  # noqa: F401
    with FakeTensorMode():
        B, E = 6, 16
        q, sp, T = torch.empty(B, E, dtype=dtype, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, B, device="cuda")
        loss, stats, gq, gdp, gdn, gsp = torch.ops.mm_native.inbatch_dot_loss(q, q, q, sp, T, T, inbatch.PAIR, _lib.PAIR_MARGIN_MSE)
        assert loss.shape == () and loss.dtype == stats.dtype == torch.float32 and stats.shape == (3,)
        assert gq.shape == gdp.shape == gdn.shape == (B, E) and gq.dtype == gdp.dtype == gdn.dtype == dtype
        assert gsp.shape == (B,) and gsp.dtype == torch.float32 and loss.device.type == "cuda"
        loss, stats, gq, gdp, gdn, gsp = torch.ops.mm_native.inbatch_dot_loss(q, q, q, sp.to(dtype), None, None, inbatch.PAIR, _lib.PAIR_RANKNET)
        assert gsp.dtype == dtype and loss.shape == ()
        S = torch.empty(B, B, dtype=dtype, device="cuda")
        loss, stats, gsp, gSp, gSn = torch.ops.mm_native.inbatch_select_loss(sp.to(dtype), S, S, T, T, inbatch.LIST, _lib.LIST_KLDIV)
        assert loss.shape == () and stats.shape == (3,) and gsp.shape == (B,) and gSp.shape == gSn.shape == (B, B)
        assert gsp.dtype == gSp.dtype == gSn.dtype == dtype


# ---- 7. routes that stay eager ---------------------------------------------------------------------------------------------------
def test_cpu_tensors_take_the_eager_path_and_the_wrappers_refuse_them():
    d, leaves, T, loss, stats, mod = run_module("margin_mse_3x8")
    assert mod.native and not mod.dot_route(leaves["sp"], leaves["Q"], leaves["Dp"], leaves["Dn"], *T)
    assert "DotLoss" not in type(loss.grad_fn).__name__
    with pytest.raises(_lib.NativeError):
        inbatch.inbatch_dot_loss(leaves["Q"], leaves["Dp"], leaves["Dn"], leaves["sp"], T[0], T[1], "pair", "margin_mse")
    with pytest.raises(_lib.NativeError):
        inbatch.inbatch_select_loss(leaves["sp"], T[0], T[1], T[0], T[1], "pair", "margin_mse")
    with pytest.raises(_lib.NativeError, match="unknown family"):
        inbatch.inbatch_select_loss(leaves["sp"], T[0], T[1], T[0], T[1], "triple", "margin_mse")


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it lives on the device: the route is a function of shapes, dtypes and flags alone"""
    is_cuda = True

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return super().__torch_function__(func, types, args, kwargs or {})


def _dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnDevice)


def test_refused_shapes_take_the_eager_route_and_do_not_raise():
    """E = 12 in fp16, B = 1025, 2 B > MM_LOSS_MAX_LIST: dot_route says no, and forward() runs the eager formula"""
    mse = inbatch.InBatchNegatives(losses.MSMarginLoss(), native=True)
    kl = inbatch.InBatchNegatives(losses.KLDivTeacherList(), True, native=True)
    rn = inbatch.InBatchNegatives(losses.RankNetLoss(), native=True)
    h = torch.float16

    def route(mod, B, E, dtype=torch.float32, teacher=True, spdt=torch.float32):
        v, T = _dev(B, E, dtype=dtype), (_dev(B, B) if teacher else None)
        return mod.dot_route(_dev(B, dtype=spdt), v, v, v, T, T)

    assert route(mse, 8, 16) and route(mse, 8, 16, h) and route(mse, 8, 12) and route(mse, 1024, 8) and route(mse, 8, 16, h, spdt=h)
    assert not route(mse, 8, 12, h) and not route(mse, 1025, 16) and not route(mse, 8, 4) and not route(mse, 8, 1032)
    assert route(kl, 512, 16) and not route(kl, 513, 16) and not route(kl, 8, 16, teacher=False)
    assert route(rn, 8, 16, teacher=False) and not route(rn, 8, 16) and not route(mse, 8, 16, teacher=False)
    assert not route(mse, 8, 16, torch.float64)
    T = _dev(8, 8).requires_grad_()
    assert not mse.dot_route(_dev(8), _dev(8, 16), _dev(8, 16), _dev(8, 16), T, T)      # a teacher that requires grad
    assert not inbatch.InBatchNegatives(torch.nn.MSELoss(), native=True).dot_route(_dev(8), _dev(8, 16), _dev(8, 16), _dev(8, 16), None, None)
    assert mse.scores_route(_dev(8), _dev(8, 8), _dev(8, 8), _dev(8, 8), _dev(8, 8)) and not mse.scores_route(_dev(8), _dev(8, 7), _dev(8, 7), None, None)
    # ... and on real (CPU) tensors of the refused shapes the module computes the eager result
    rng = np.random.default_rng(5)
    for mod, kind, family, B, E, dtype in ((mse, "margin_mse", "pair", 4, 12, h), (mse, "margin_mse", "pair", 1025, 8, torch.float32),
                                           (kl, "kldiv", "list", 513, 8, torch.float32)):
        f = np.float32
        sp, Q, Dp, Dn = (torch.from_numpy(f(rng.standard_normal(s))).to(dtype).float() for s in ((B,), (B, E), (B, E), (B, E)))
        Tp, Tn = torch.from_numpy(f(rng.standard_normal((B, B)))), torch.from_numpy(f(rng.standard_normal((B, B))))
        loss, stats = mod(sp, Q, Dp, Dn, Tp, Tn)
        n, M2, _ = IR.counts(sp.numpy(), (Q @ Dp.T).numpy(), (Q @ Dn.T).numpy())
        assert torch.isfinite(loss) and round(float(stats["accuracy"]) * M2) == n
