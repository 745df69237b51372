"""CPU tests of the native training losses (matchmaker_amd/losses.py over csrc/losses.hip): the float64 restatement against the
goldens recorded from the real reference classes, the module's eager formulas against the reference (live where its tree is
found, else the goldens), get_loss, patch_losses, the C boundary's refusals and the fake implementations of the torch ops."""
import re
import sys
import types
import warnings

import numpy as np
import pytest
import torch

from matchmaker_amd import _lib, losses, patch
from oracle import ref_harness
from tests import abi, losses_reference as R, util

PAIRS = util.load("losses_pairs.npz")
LISTS = util.load("losses_lists.npz")
CLASS = {"ranknet": losses.RankNetLoss, "margin": losses.MarginRankingLoss1, "margin_mse": losses.MSMarginLoss,
         "mse_pointwise": losses.MSETeacherPointwise, "kldiv_pointwise": losses.KLDivTeacherPointwise,
         "ranknet_teacher": losses.RankNetTeacher, "mse_ranknet": losses.MSERanknetTeacher, "listnet": losses.ListNetLoss,
         "kldiv": losses.KLDivTeacherList, "smooth_mrr": losses.SmoothMRRLoss,
         "lambda_ndcg2": lambda: losses.LambdaLoss("ndcgLoss2_scheme"),
         "lambda_ndcg2_teacher": lambda: losses.LambdaLossTeacher("ndcgLoss2_scheme")}


def pair_labels(kind, d=PAIRS):
    return {"ranknet": (d["y01"],), "margin": (d["ysign"],)}.get(kind, (d["a"], d["b"]))


def list_labels(kind, L, d=LISTS):
    return d[f"grades_{L}"] if kind == "lambda_ndcg2" else d[f"smooth_mrr_{L}.labels"] if kind == "smooth_mrr" else d[f"labels_{L}"]


def close32(got, want, scale=None, ulps=64):
    """fp32-class agreement: within `ulps` fp32 ulps of the largest magnitude (sums of <= 70^2 fp32 terms on both sides)"""
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if scale is None else scale
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() <= ulps * R.ulp32(max(scale, 1e-30))


# ---- 1. the float64 restatement agrees with the goldens ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PAIR_KINDS)
def test_restatement_matches_the_pair_goldens(kind):
    loss, gp, gn = R.pair(kind, PAIRS["pos"], PAIRS["neg"], *pair_labels(kind))
    assert close32(PAIRS[kind + ".loss"], loss)
    assert close32(PAIRS[kind + ".gpos"], gp) and close32(PAIRS[kind + ".gneg"], gn)


@pytest.mark.parametrize("L", (17, 70))
@pytest.mark.parametrize("kind", R.LIST_KINDS)
def test_restatement_matches_the_list_goldens(kind, L):
    loss, per, grad = R.lists(kind, LISTS[f"scores_{L}"], list_labels(kind, L))
    assert close32(LISTS[f"{kind}_{L}.loss"], loss)
    assert close32(LISTS[f"{kind}_{L}.grad"], grad)
    if kind == "smooth_mrr":
        assert close32(LISTS[f"smooth_mrr_{L}.per_list"], per)
    if kind == "lambda_ndcg2":      # the fully padded list: term 0, gradient 0
        assert per[2] == 0 and not grad[2].any() and not LISTS[f"lambda_ndcg2_{L}.grad"][2].any()


# ---- 2. the module's eager formulas agree with the reference ----------------------------------------------------------------
def _reference_class(kind):
    if ref_harness.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REFERENCE_ROOT)
    import importlib
    mod, name = {"ranknet": ("ranknet", "RankNetLoss"), "margin_mse": ("msmargin", "MSMarginLoss"),
                 "mse_pointwise": ("teacher_mse_pointwise", "MSETeacherPointwise"),
                 "kldiv_pointwise": ("teacher_kldiv_pointwise", "KLDivTeacherPointwise"),
                 "ranknet_teacher": ("teacher_ranknetweighted", "RankNetTeacher"),
                 "mse_ranknet": ("teacher_mse_ranknet", "MSERanknetTeacher"), "listnet": ("listnet", "ListNetLoss"),
                 "kldiv": ("teacher_kldiv_list", "KLDivTeacherList"), "smooth_mrr": ("loss_smooth_mrr", "SmoothMRRLoss"),
                 "lambda_ndcg2": ("lambdarank", "LambdaLoss"), "lambda_ndcg2_teacher": ("lambdarank", "LambdaLossTeacher")}[kind]
    cls = getattr(importlib.import_module("matchmaker.losses." + mod), name)
    return (lambda: cls("ndcgLoss2_scheme")) if kind.startswith("lambda") else cls


def _run(mod, scores, labels, **kw):
    leaves = [torch.from_numpy(np.array(s)).requires_grad_() for s in scores]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = mod(*[t * 1.0 for t in leaves], *[torch.from_numpy(np.array(t)) for t in labels], **kw)
    loss.backward()
    return [loss.detach().numpy()] + [t.grad.numpy() for t in leaves]


@pytest.mark.parametrize("kind", R.PAIR_KINDS)
def test_eager_pair_formulas_match_the_reference(kind):
    got = _run(CLASS[kind](), (PAIRS["pos"], PAIRS["neg"]), pair_labels(kind))
    want = [PAIRS[kind + ".loss"], PAIRS[kind + ".gpos"], PAIRS[kind + ".gneg"]]
    if ref_harness.available() and kind != "margin":      # ("margin" is torch's own class in the reference)
        want = _run(_reference_class(kind)(), (PAIRS["pos"], PAIRS["neg"]), pair_labels(kind))
    for g, w in zip(got, want):
        assert close32(g, w, ulps=4)


@pytest.mark.parametrize("L", (17, 70))
@pytest.mark.parametrize("kind", R.LIST_KINDS)
def test_eager_list_formulas_match_the_reference(kind, L):
    scores, labels = LISTS[f"scores_{L}"], list_labels(kind, L)
    got = _run(CLASS[kind](), (scores,), (labels,))
    want = [LISTS[f"{kind}_{L}.loss"], LISTS[f"{kind}_{L}.grad"]]
    if ref_harness.available():
        want = _run(_reference_class(kind)(), (scores,), (labels,))
    for g, w in zip(got, want):
        assert close32(g, w, ulps=4)
    if kind == "smooth_mrr":
        per = CLASS[kind]()(torch.from_numpy(scores), torch.from_numpy(labels), agg=False)
        assert close32(per.numpy(), LISTS[f"smooth_mrr_{L}.per_list"], ulps=4)


def test_eager_lambda_leaves_its_inputs_alone():
    s, y = torch.from_numpy(LISTS["scores_17"].copy()), torch.from_numpy(LISTS["grades_17"].copy())
    losses.LambdaLoss("ndcgLoss2_scheme")(s, y)
    assert torch.equal(s, torch.from_numpy(LISTS["scores_17"])) and torch.equal(y, torch.from_numpy(LISTS["grades_17"]))


# ---- 3. get_loss ------------------------------------------------------------------------------------------------------------
MAIN = {"margin-mse": (losses.MSMarginLoss, False), "MSETeacherPointwise": (losses.MSETeacherPointwise, False),
        "KLDivTeacherPointwise": (losses.KLDivTeacherPointwise, False), "RankNetTeacher": (losses.RankNetTeacher, False),
        "MSERanknetTeacher": (losses.MSERanknetTeacher, False), "ranknet": (losses.RankNetLoss, False),
        "margin": (losses.MarginRankingLoss1, False), "mrr": (losses.SmoothMRRLoss, True), "listnet": (losses.ListNetLoss, True),
        "lambdarank": (losses.LambdaLoss, True)}
INBATCH = {"ranknet": (losses.RankNetLoss, False), "margin-mse": (losses.MSMarginLoss, False),
           "KLDivTeacherList": (losses.KLDivTeacherList, True), "listnet": (losses.ListNetLoss, True),
           "lambdarank": (losses.LambdaLossTeacher, True)}


def _config(loss, inbatch=None, qa=None):
    return {"loss": loss, "train_qa_spans": qa is not None, "qa_loss": qa, "in_batch_negatives": inbatch is not None,
            "in_batch_neg_loss": inbatch}


@pytest.mark.parametrize("name", sorted(MAIN))
def test_get_loss_main_names(name):
    loss, qa, ib, use_list, use_ib_list = losses.get_loss(_config(name))
    assert type(loss) is MAIN[name][0] and qa is None and ib is None and use_list is MAIN[name][1] and use_ib_list is False
    if name == "lambdarank":
        assert loss.weighing_scheme == "ndcgLoss2_scheme"
    if name == "margin":
        assert isinstance(loss, torch.nn.MarginRankingLoss) and loss.margin == 1 and loss.reduction == "mean"


@pytest.mark.parametrize("name", sorted(INBATCH))
def test_get_loss_inbatch_names(name):
    loss, qa, ib, use_list, use_ib_list = losses.get_loss(_config("margin-mse", inbatch=name))
    assert type(loss) is losses.MSMarginLoss and type(ib) is INBATCH[name][0] and use_ib_list is INBATCH[name][1]
    assert type(ib) is not losses.LambdaLossTeacher or ib.weighing_scheme == "ndcgLoss2_scheme"


def test_get_loss_names_it_does_not_restate():
    with pytest.raises(Exception, match="Loss not known.*nonsense"):
        losses.get_loss(_config("nonsense"))
    with pytest.raises(Exception, match="In-batch-Loss not known.*nonsense"):
        losses.get_loss(_config("margin-mse", inbatch="nonsense"))
    with pytest.raises(Exception, match="QA-Loss not known.*nonsense"):
        losses.get_loss(_config("margin-mse", qa="nonsense"))
    for name in ("MSETeacherPointwisePassages", "MarginMSE_InterPassageLoss"):
        if ref_harness.available():
            ref_harness.install_shims()
            assert type(losses.get_loss(_config(name))[0]).__name__ == name
        else:
            with pytest.raises(Exception, match="Loss not known.*" + name):
                losses.get_loss(_config(name))


@pytest.mark.skipif(not ref_harness.available(), reason="needs the reference tree")
def test_get_loss_matches_the_reference_tuple():
    ref_harness.install_shims()
    from matchmaker.losses.all import get_loss as ref_get_loss
    for name in MAIN:
        if name == "mrr":      # all.py never imports loss_smooth_mrr: the reference's own get_loss raises NameError for "mrr"
            with pytest.raises(NameError):
                ref_get_loss(_config(name))
            continue
        for ib in (None,) + tuple(INBATCH):
            ours, theirs = losses.get_loss(_config(name, ib)), ref_get_loss(_config(name, ib))
            assert ours[3:] == theirs[3:] and (ours[1] is None) == (theirs[1] is None)
            for o, t in ((ours[0], theirs[0]), (ours[2], theirs[2])):
                assert (o is None) == (t is None)
                if o is not None and name != "margin":
                    assert type(o).__name__ == type(t).__name__
                    assert getattr(o, "weighing_scheme", None) == getattr(t, "weighing_scheme", None)


# ---- 4. patch_losses ----------------------------------------------------------------------------------------------------------
def test_patch_losses_rebinds_and_patch_matchmaker_does_not(monkeypatch):
    """on stand-ins under the reference's module names (sys.modules is consulted first, so the real tree is never touched by
    patch_losses here); patch_matchmaker() runs on whatever the process holds, and its rebinding is undone afterwards"""
    import importlib
    names = {m for m, _, _ in patch._LOSS_TABLE} | {"matchmaker.losses.all"}
    fakes = {n: types.ModuleType(n) for n in names}
    for mod, attr, _ in patch._LOSS_TABLE:
        setattr(fakes[mod], attr, object())
        if attr != "SmoothMRRLoss":      # (all.py never imports loss_smooth_mrr)
            setattr(fakes["matchmaker.losses.all"], attr, getattr(fakes[mod], attr))
    fakes["matchmaker.losses.all"].get_loss = object()
    for n, m in fakes.items():
        monkeypatch.setitem(sys.modules, n, m)
    saved = {}
    for ref_mod, ref_attr, _, _ in patch._TABLE:
        try:
            saved[(ref_mod, ref_attr)] = getattr(importlib.import_module(ref_mod), ref_attr)
        except Exception:
            pass
    try:
        before = patch.patch_matchmaker()
        assert not any("losses" in d for d in before) and set(before) <= {m + "." + a for m, a, _, _ in patch._TABLE}
        assert fakes["matchmaker.losses.msmargin"].MSMarginLoss is not losses.MSMarginLoss      # the models' patch left the losses alone
        assert fakes["matchmaker.losses.all"].get_loss is not losses.get_loss
        done = patch.patch_losses()
        assert len(done) == len(patch._LOSS_TABLE) + 1 and done[-1] == "matchmaker.losses.all.get_loss"
        for mod, attr, ours in patch._LOSS_TABLE:
            assert getattr(fakes[mod], attr) is getattr(losses, ours)
            assert attr == "SmoothMRRLoss" or getattr(fakes["matchmaker.losses.all"], attr) is getattr(losses, ours)
        assert not hasattr(fakes["matchmaker.losses.all"], "SmoothMRRLoss")
        assert fakes["matchmaker.losses.all"].get_loss is losses.get_loss
        assert patch.patch_matchmaker() == before and all(len(row) == 4 for row in patch._TABLE) and len(patch._TABLE) == 11
    finally:                                             # other tests drive the real classes
        for (ref_mod, ref_attr), obj in saved.items():
            setattr(importlib.import_module(ref_mod), ref_attr, obj)


# ---- 5. symbols, header, ABI version -------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_the_header_cites_what_it_replaces():
    L = abi.assert_bound(("mm_pair_loss_fwd", "mm_pair_loss_workspace_bytes", "mm_list_loss_fwd"))
    assert _lib.ABI_VERSION == 4 == L.mm_abi_version()
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for entry in ("mm_pair_loss_fwd", "mm_list_loss_fwd"):
        block = text[text.index(entry + " (additive: MM_ABI_VERSION unchanged)"):]
        block = block[:block.index("*/")]
        assert re.search(r"Replaces: matchmaker/losses/\w+\.py:\d+", block), entry
    for f in ("ranknet.py:15-16", "all.py:48", "msmargin.py:13", "teacher_mse_pointwise.py:13-14", "teacher_kldiv_pointwise.py:13-14",
              "teacher_ranknetweighted.py:16-18", "teacher_mse_ranknet.py:13-15", "listnet.py:27-33", "teacher_kldiv_list.py:13",
              "loss_smooth_mrr.py:11-33", "lambdarank.py:65-119"):
        assert "matchmaker/losses/" + f in text, f
    assert [_lib.PAIR_RANKNET, _lib.PAIR_MARGIN, _lib.PAIR_MARGIN_MSE, _lib.PAIR_MSE_POINTWISE, _lib.PAIR_KLDIV_POINTWISE,
            _lib.PAIR_RANKNET_TEACHER, _lib.PAIR_MSE_RANKNET] == list(range(7))
    assert [_lib.LIST_LISTNET, _lib.LIST_KLDIV, _lib.LIST_SMOOTH_MRR, _lib.LIST_LAMBDA_NDCG2, _lib.LIST_LAMBDA_NDCG2_TEACHER] == list(range(5))
    assert _lib.LOSS_MAX_LIST == losses.MAX_LIST == 1024


# ---- 6. refusals of the C boundary (before any launch: no device needed) -------------------------------------------------------
def test_c_abi_refusals_need_no_device():
    L = abi.assert_bound(("mm_pair_loss_fwd", "mm_list_loss_fwd"))
    p = 4096      # never dereferenced: every call below is refused first
    pair = lambda n, kind, dtype=_lib.MM_F32, loss=p, a=p: L.mm_pair_loss_fwd(p, p, dtype, a, p, n, kind, loss, p, p, None, 0, None)  # noqa: E731
    assert pair(-1, _lib.PAIR_MARGIN_MSE) == _lib.MM_EINVAL and b"n=-1" in L.mm_last_error()
    assert pair(8, 7) == _lib.MM_EINVAL and pair(8, -1) == _lib.MM_EINVAL
    assert pair(8, _lib.PAIR_MARGIN_MSE, dtype=3) == _lib.MM_EINVAL
    assert pair(8, _lib.PAIR_MARGIN_MSE, loss=None) == _lib.MM_EINVAL and pair(8, _lib.PAIR_MARGIN_MSE, a=None) == _lib.MM_EINVAL
    assert pair(2 ** 31 + 1, _lib.PAIR_MARGIN_MSE) == _lib.MM_EUNSUPPORTED
    assert pair(70000, _lib.PAIR_MARGIN_MSE) == _lib.MM_EWORKSPACE      # more than one workgroup's share and no workspace
    assert L.mm_pair_loss_workspace_bytes(4096) == 0 and L.mm_pair_loss_workspace_bytes(70000) == 18 * 8
    assert L.mm_pair_loss_workspace_bytes(2 ** 31) == 1024 * 8
    lst = lambda B, Ln, kind, dtype=_lib.MM_F32, loss=p: L.mm_list_loss_fwd(p, dtype, p, B, Ln, kind, loss, p, p, None)  # noqa: E731
    assert lst(-1, 8, 0) == _lib.MM_EINVAL and lst(8, -1, 0) == _lib.MM_EINVAL
    assert lst(8, 8, 5) == _lib.MM_EINVAL and lst(8, 8, -1) == _lib.MM_EINVAL and lst(8, 8, 0, dtype=7) == _lib.MM_EINVAL
    assert lst(8, 8, 0, loss=None) == _lib.MM_EINVAL
    assert lst(8, 1025, _lib.LIST_LAMBDA_NDCG2) == _lib.MM_EUNSUPPORTED and b"1025" in L.mm_last_error()


# ---- 7. fake implementations of the torch ops ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16, torch.bfloat16))
def test_fake_shapes_and_dtypes(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import matchmaker_amd.torch_ops  # noqa: F401
    with FakeTensorMode():
        pos, a = torch.empty(6, 5, dtype=dtype, device="cuda"), torch.empty(6, 5, device="cuda")
        loss, gp, gn = torch.ops.mm_native.pair_loss(pos, pos, a, a, _lib.PAIR_MARGIN_MSE)
        assert loss.shape == () and loss.dtype == torch.float32 and gp.shape == gn.shape == (6, 5) and gp.dtype == gn.dtype == dtype
        loss, gp, gn = torch.ops.mm_native.pair_loss(pos, pos, a, None, _lib.PAIR_RANKNET)
        assert loss.shape == () and gp.shape == (6, 5)
        loss, per, grad = torch.ops.mm_native.list_loss(pos, a, _lib.LIST_LISTNET)
        assert loss.shape == () and loss.dtype == per.dtype == torch.float32 and per.shape == (6,)
        assert grad.shape == (6, 5) and grad.dtype == dtype and loss.device.type == "cuda"


# ---- 8. routes that stay eager ---------------------------------------------------------------------------------------------------
def test_cpu_tensors_take_the_eager_path():
    for kind in R.PAIR_KINDS:      # native = True and CPU tensors: a native call would raise NativeError
        mod = CLASS[kind]()
        mod.native = True
        got = _run(mod, (PAIRS["pos"], PAIRS["neg"]), pair_labels(kind))
        assert close32(got[0], PAIRS[kind + ".loss"], ulps=4)
    with pytest.raises(_lib.NativeError):
        losses.pair_loss(torch.zeros(3), torch.zeros(3), torch.zeros(3), torch.zeros(3), "margin_mse")
    with pytest.raises(_lib.NativeError):
        losses.list_loss(torch.zeros(3, 3), torch.zeros(3, 3), "listnet")


@pytest.mark.parametrize("i", range(len(R.LAMBDA_ARG_CASES)))
def test_unsupported_lambda_arguments_run_the_eager_formula_and_match_the_reference(i):
    """against the live reference class where its tree is found, else against its recorded result"""
    scheme, kw = R.LAMBDA_ARG_CASES[i]
    scores, grades = LISTS["scores_17"], LISTS["grades_17"]
    want = [LISTS[f"lambda_args_{i}.loss"], LISTS[f"lambda_args_{i}.grad"]]
    if ref_harness.available():
        if ref_harness.REFERENCE_ROOT not in sys.path:
            sys.path.insert(0, ref_harness.REFERENCE_ROOT)
        from matchmaker.losses.lambdarank import LambdaLoss as RefLambda
        live = _run(RefLambda(scheme), (scores,), (grades,), **kw)
        assert all(np.array_equal(a, b) for a, b in zip(live, want)), "the golden is the reference's own result"
    mod = losses.LambdaLoss(scheme)
    assert not mod._native_args(kw.get("padded_value_indicator", -1), kw.get("eps", 1e-6), kw.get("k"), kw.get("sigma", 1.),
                                kw.get("reduction", "sum"), kw.get("reduction_log", "binary"))
    got = _run(mod, (scores,), (grades,), **kw)
    for g, w in zip(got, want):
        assert close32(g, w, ulps=4)
    with pytest.raises(ValueError):
        mod(torch.from_numpy(scores), torch.from_numpy(grades), reduction="median")


def test_native_defaults_follow_the_measured_rule():
    """True only where native beat eager in every leg by more than the spread of two rounds, in every measured run"""
    want = {k: True for k in CLASS}
    want["ranknet"] = want["margin_mse"] = False
    assert {k: CLASS[k]().native for k in CLASS} == want
