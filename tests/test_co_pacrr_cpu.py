"""CPU tests of CO-PACRR (no GPU): the fp64 restatement (tests/co_pacrr_reference.py) against the real class's goldens and,
where the reference tree exists, against live instances; the drop-in's from_config / state_dict parity; patch_matchmaker's
rebinding; the fake (meta) implementation of torch.ops.mm_native.co_pacrr_kmax; the host and C ABI refusals (no device
needed)."""
import sys
import types

import numpy as np
import pytest
import torch

from oracle import ref_harness as R
from tests import co_pacrr_reference as CP
from tests import util

CFG = {"pacrr_unified_query_length": 30, "pacrr_unified_document_length": 200, "pacrr_max_conv_kernel_size": 3,
       "pacrr_conv_output_size": 32, "pacrr_kmax_pooling_size": 5}       # config/train/non-bert-defaults.yaml:54-58
CASES = ["ref", "short", "mid", "long", "oddu", "padded", "qpad", "b1", "n1", "k1"]
# padded query rows tie across their whole row: which columns (and so which contexts) the real class's torch.topk keeps
# there is implementation-defined, and the dense layers carry that choice into the score and every gradient
TIE_DEPENDENT = {"qpad"}


def _dense(g):
    return [torch.tensor(g["param." + k], dtype=torch.float64)
            for k in ("dense.weight", "dense.bias", "dense2.weight", "dense2.bias", "dense3.weight")]


def _restated(g):
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    q = torch.tensor(g["q"], dtype=torch.float64, requires_grad=True)
    d = torch.tensor(g["d"], dtype=torch.float64, requires_grad=True)
    ws = [torch.tensor(g[f"param.convolutions.{i}.1.weight"], dtype=torch.float64, requires_grad=True) for i in range(N - 1)]
    bs = [torch.tensor(g[f"param.convolutions.{i}.1.bias"], dtype=torch.float64, requires_grad=True) for i in range(N - 1)]
    pqr = CP.per_query_results(q, d, ws, bs, k, int(g["U"]))
    s = CP.score(pqr, *_dense(g))
    s.sum().backward()
    return q, d, ws, bs, pqr, s


def _value_mask(k, N):
    m = torch.zeros(8 * k * N, dtype=torch.bool)
    for p in range(N):
        m[p * 8 * k:p * 8 * k + 4 * k] = True
    return m


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_real_class_goldens(name):
    g = util.load(f"co_pacrr_{name}.npz")
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    q, d, ws, bs, pqr, s = _restated(g)
    ref = torch.tensor(g["per_query_results"])
    vm = _value_mask(k, N)
    np.testing.assert_allclose(pqr.detach()[..., vm].numpy(), ref[..., vm].numpy(), rtol=0, atol=2e-5)
    mats = CP.paths(q.detach(), d.detach(), [w.detach() for w in ws], [b.detach() for b in bs])
    excluded = CP.compare_context_slots(ref, pqr, mats, k, int(g["U"]), atol=2e-5)
    print(f"co_pacrr_{name}: {excluded} context slots excluded (tied groups across the k-th place)")
    if name in TIE_DEPENDENT:
        assert excluded > 0
        return
    np.testing.assert_allclose(s.detach().numpy(), g["score"], rtol=1e-5, atol=1e-5)
    for i in range(N - 1):
        np.testing.assert_allclose(ws[i].grad.numpy(), g[f"grad.convolutions.{i}.1.weight"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(bs[i].grad.numpy(), g[f"grad.convolutions.{i}.1.bias"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(q.grad.numpy(), g["grad_q"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(d.grad.numpy(), g["grad_d"], rtol=1e-4, atol=1e-4)


def _reference_class(monkeypatch):
    """The real CO_PACRR class, imported with co_pacrr.py's allennlp imports stubbed through monkeypatch (sys.modules is
    restored afterwards)."""
    R.install_shims()
    nn_mod = types.ModuleType("allennlp.nn")
    util_mod = types.ModuleType("allennlp.nn.util")
    util_mod.get_text_field_mask = lambda *a, **kw: None
    nn_mod.util = util_mod
    monkeypatch.setitem(sys.modules, "allennlp.nn", nn_mod)
    monkeypatch.setitem(sys.modules, "allennlp.nn.util", util_mod)
    dp = types.ModuleType("allennlp.modules.matrix_attention.dot_product_matrix_attention")
    dp.DotProductMatrixAttention = torch.nn.Module
    monkeypatch.setitem(sys.modules, "allennlp.modules.matrix_attention.dot_product_matrix_attention", dp)
    monkeypatch.delitem(sys.modules, "matchmaker.models.co_pacrr", raising=False)
    import importlib
    return importlib.import_module("matchmaker.models.co_pacrr").CO_PACRR


@pytest.mark.skipif(not R.available(), reason="live parity needs the reference tree; the goldens cover the rest")
@pytest.mark.parametrize("Q, U, D, E, N, C, k", [(30, 200, 200, 64, 3, 32, 5), (7, 40, 33, 24, 4, 8, 3),
                                                 (12, 30, 50, 32, 1, 16, 2)])
def test_restatement_matches_the_live_class_forward_and_autograd(monkeypatch, Q, U, D, E, N, C, k):
    Ref = _reference_class(monkeypatch)
    torch.manual_seed(Q + D)
    m = Ref(unified_query_length=Q, unified_document_length=U, max_conv_kernel_size=N, conv_output_size=C,
            kmax_pooling_size=k).double().eval()
    B = 3
    q = torch.randn(B, Q, E, dtype=torch.float64, requires_grad=True)
    d = torch.randn(B, D, E, dtype=torch.float64, requires_grad=True)
    s = m(q, d, torch.ones(B, Q), torch.ones(B, D), torch.ones(B, Q, 1), torch.ones(B, D, 1))
    s.sum().backward()
    q2 = q.detach().clone().requires_grad_(True)
    d2 = d.detach().clone().requires_grad_(True)
    ws = [c[1].weight.detach().clone().requires_grad_(True) for c in m.convolutions]
    bs = [c[1].bias.detach().clone().requires_grad_(True) for c in m.convolutions]
    s2 = CP.score(CP.per_query_results(q2, d2, ws, bs, k, U), m.dense.weight, m.dense.bias, m.dense2.weight,
                  m.dense2.bias, m.dense3.weight)
    s2.sum().backward()
    torch.testing.assert_close(s2, s, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(q2.grad, q.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(d2.grad, d.grad, rtol=1e-10, atol=1e-10)
    for w, b, c in zip(ws, bs, m.convolutions):
        torch.testing.assert_close(w.grad, c[1].weight.grad, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(b.grad, c[1].bias.grad, rtol=1e-10, atol=1e-10)


def test_from_config_and_state_dict_match_the_real_class(monkeypatch):
    from matchmaker_amd.co_pacrr import CO_PACRR
    mine = CO_PACRR.from_config(CFG, 300)
    g = util.load("co_pacrr_ref.npz")
    keys = sorted(k[len("param."):] for k in g if k.startswith("param."))
    assert sorted(mine.state_dict()) == keys
    mine.load_state_dict({k: torch.tensor(g["param." + k]) for k in keys}, strict=True)
    assert mine.kmax_pooling_views == [50, 100, 150, 200] and mine.dense.in_features == 3600
    assert [type(c[i]).__name__ for c in mine.convolutions for i in range(3)] == ["ConstantPad2d", "Conv2d", "MaxPool3d"] * 2
    assert [type(m).__name__ for m in mine.doc_context_pool] == ["ConstantPad1d", "AvgPool1d"]
    assert mine.get_param_stats() == "CO-PACRR: / " and mine.get_param_secondary() == {}
    assert CO_PACRR(30, 30, 3, 32, 5).kmax_pooling_views == [7, 15, 22, 30]
    if R.available():
        Ref = _reference_class(monkeypatch)
        ref = Ref.from_config(CFG, 300)
        assert {k: v.shape for k, v in ref.state_dict().items()} == {k: v.shape for k, v in mine.state_dict().items()}
        assert sorted(n for n, _ in ref.named_parameters()) == sorted(n for n, _ in mine.named_parameters())
        mine.load_state_dict(ref.state_dict(), strict=True)
        ref.load_state_dict(mine.state_dict(), strict=True)
        for U in (200, 30, 16, 333):
            assert Ref(30, U, 3, 32, 5).kmax_pooling_views == CO_PACRR(30, U, 3, 32, 5).kmax_pooling_views
        x = torch.randn(4, 30, 1)
        mask = (torch.rand(4, 30, 1) > 0.3).float()
        mask[:, 0] = 1.0
        torch.testing.assert_close(mine.masked_softmax(x, mask), ref.masked_softmax(x, mask))


def test_patch_matchmaker_rebinds_co_pacrr(monkeypatch):
    """on the real module where the reference tree is present, on a stand-in with the same name otherwise"""
    from matchmaker_amd import patch
    from matchmaker_amd.co_pacrr import CO_PACRR
    assert ("matchmaker.models.co_pacrr", "CO_PACRR", "matchmaker_amd.co_pacrr", "CO_PACRR") in patch._TABLE
    if R.available():
        Ref = _reference_class(monkeypatch)
        ref_mod = sys.modules["matchmaker.models.co_pacrr"]
    else:
        for name in ("matchmaker", "matchmaker.models", "matchmaker.models.published"):
            monkeypatch.setitem(sys.modules, name, sys.modules.get(name) or types.ModuleType(name))
        ref_mod = types.ModuleType("matchmaker.models.co_pacrr")
        Ref = type("CO_PACRR", (), {})
        ref_mod.CO_PACRR = Ref
        monkeypatch.setitem(sys.modules, "matchmaker.models.co_pacrr", ref_mod)
    all_mod = types.ModuleType("matchmaker.models.all")
    all_mod.CO_PACRR = Ref
    monkeypatch.setitem(sys.modules, "matchmaker.models.all", all_mod)
    import importlib
    for mod_name, attr, _, _ in patch._TABLE:           # every rebinding is undone afterwards
        try:
            mod = importlib.import_module(mod_name)
        except Exception:
            continue
        monkeypatch.setattr(mod, attr, getattr(mod, attr))
    monkeypatch.setattr(patch, "_idcm_note_given", True)
    done = patch.patch_matchmaker()
    assert "matchmaker.models.co_pacrr.CO_PACRR" in done
    assert ref_mod.CO_PACRR is CO_PACRR and all_mod.CO_PACRR is CO_PACRR
    m = all_mod.CO_PACRR.from_config(CFG, 300)          # models/all.py:163
    assert type(m).__module__ == "matchmaker_amd.co_pacrr"


@pytest.mark.parametrize("nq, ppq, B, N, k", [(4, 1, 4, 3, 5), (2, 1000, 1500, 3, 5), (3, 1, 3, 1, 2), (1, 1, 1, 5, 8)])
def test_fake_tensor_shapes_of_the_torch_op(nq, ppq, B, N, k):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from matchmaker_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        q = torch.empty(nq, 30, 300, device="cuda")
        d = torch.empty(B, 200, 300, device="cuda")
        ws = [torch.empty(32, 1, n, n, device="cuda") for n in range(2, N + 1)]
        bs = [torch.empty(32, device="cuda") for _ in range(2, N + 1)]
        out, idx = torch.ops.mm_native.co_pacrr_kmax(q, d, ws, bs, k, [50, 100, 150, 200], ppq)
        assert tuple(out.shape) == (B, 30, 8 * k * N) and out.dtype == torch.float32
        assert tuple(idx.shape) == (B, 30, N, 4 * k) and idx.dtype == torch.int32
        gq, gd, gw, gb = torch.ops.mm_native.co_pacrr_kmax_backward(q, d, ws, idx, out, k, [50, 100, 150, 200], ppq)
        assert tuple(gq.shape) == tuple(q.shape) and tuple(gd.shape) == tuple(d.shape)
        assert [tuple(t.shape) for t in gw] == [tuple(w.shape) for w in ws] and [tuple(t.shape) for t in gb] == [(32,)] * (N - 1)


def test_autograd_rule_shapes_on_meta_tensors():
    from matchmaker_amd import torch_ops  # noqa: F401
    q = torch.empty(2, 30, 64, device="meta", requires_grad=True)
    d = torch.empty(4, 200, 64, device="meta", requires_grad=True)
    ws = [torch.empty(32, 1, n, n, device="meta", requires_grad=True) for n in (2, 3)]
    bs = [torch.empty(32, device="meta", requires_grad=True) for _ in (2, 3)]
    for ppq in (2, 1):
        out, idx = torch.ops.mm_native.co_pacrr_kmax(q, d[:2 * ppq], ws, bs, 5, [50, 100, 150, 200], ppq)
        out.sum().backward()
    assert q.grad.shape == q.shape and d.grad.shape == d.shape
    assert [w.grad.shape for w in ws] == [w.shape for w in ws] and [b.grad.shape for b in bs] == [b.shape for b in bs]


def test_ops_reject_cpu_tensors_and_out_of_limit_shapes():
    from matchmaker_amd import ops, NativeError
    q, d = torch.zeros(1, 4, 16), torch.zeros(1, 60, 16)
    with pytest.raises(NativeError):
        ops.co_pacrr_kmax(q, d, [], [], 5, ops.co_pacrr_views(200))
    with pytest.raises(NativeError):
        ops.co_pacrr_kmax_bwd(q, d, [], torch.zeros(1, 4, 1, 20, dtype=torch.int32), torch.zeros(1, 4, 40), 5,
                              ops.co_pacrr_views(200))


def test_views_narrower_than_k_are_refused_as_the_reference_raises(monkeypatch):
    """int(U * 0.25) < k: torch.topk raises in the reference (U = 16, k = 5 even for D = 40); the host refuses the shape
    before it looks at the device (meta tensors here), and the C entry returns MM_EUNSUPPORTED (C client test)."""
    from matchmaker_amd import ops, NativeError
    assert ops.co_pacrr_views(16) == [4, 8, 12, 16]
    with pytest.raises(NativeError, match="views"):
        ops._co_pacrr_check(2, 30, 40, 64, 5, ops.co_pacrr_views(16))
    ops._co_pacrr_check(2, 30, 40, 64, 5, ops.co_pacrr_views(20))          # views 5 / 10 / 15 / 20: fine
    with pytest.raises(NativeError):
        ops._co_pacrr_check(2, 30, 40, 64, 5, [10, 5, 15, 20])             # not ascending
    if R.available():
        Ref = _reference_class(monkeypatch)
        m = Ref(30, 16, 3, 8, 5)
        B = 2
        with pytest.raises(RuntimeError):
            m(torch.randn(B, 30, 16), torch.randn(B, 40, 16), torch.ones(B, 30), torch.ones(B, 40), torch.ones(B, 30, 1),
              torch.ones(B, 40, 1))


def test_c_client_gets_einval_and_eunsupported_without_a_gpu(tmp_path):
    from tests import abi
    out = abi.run_c_client(tmp_path, r"""
#include <stdio.h>
#include <string.h>
#include "mm_native.h"
static float f[4];
static int32_t ix[4];
int main(void) {
  /* null pointers: refused before anything touches the device */
  if (mm_co_pacrr_fwd(NULL, f, f, f, f, NULL, 4, 1, 30, 200, 300, 32, 3, 5, 50, 100, 150, 200, NULL, 0, NULL) != MM_EINVAL) return 1;
  if (mm_co_pacrr_fwd(f, f, NULL, f, f, NULL, 4, 1, 30, 200, 300, 32, 3, 5, 50, 100, 150, 200, NULL, 0, NULL) != MM_EINVAL) return 2;
  if (mm_co_pacrr_bwd(f, f, f, NULL, f, f, f, f, f, 4, 1, 30, 200, 300, 32, 3, 5, 50, 100, 150, 200, NULL, 0, NULL) != MM_EINVAL) return 3;
  if (mm_co_pacrr_bwd(f, f, f, ix, f, NULL, f, f, f, 4, 1, 30, 200, 300, 32, 3, 5, 50, 100, 150, 200, NULL, 0, NULL) != MM_EINVAL) return 4;
  if (strlen(mm_last_error()) == 0) return 5;
  /* views not ascending */
  if (mm_co_pacrr_fwd(f, f, f, f, f, ix, 4, 1, 30, 200, 300, 32, 3, 5, 100, 50, 150, 200, NULL, 0, NULL) != MM_EINVAL) return 6;
  /* outside the limits (pointers are host memory: nothing may be launched) */
  const int bad[][10] = {{65, 200, 300, 32, 3, 5, 50, 100, 150, 200}, {30, 4, 300, 32, 3, 5, 50, 100, 150, 200},
                         {30, 2049, 300, 32, 3, 5, 50, 100, 150, 200}, {30, 200, 1028, 32, 3, 5, 50, 100, 150, 200},
                         {30, 200, 302, 32, 3, 5, 50, 100, 150, 200}, {30, 200, 300, 65, 3, 5, 50, 100, 150, 200},
                         {30, 200, 300, 32, 6, 5, 50, 100, 150, 200}, {30, 200, 300, 32, 3, 9, 50, 100, 150, 200},
                         {30, 200, 300, 32, 0, 5, 50, 100, 150, 200}, {30, 200, 300, 32, 3, 0, 50, 100, 150, 200},
                         {0, 200, 300, 32, 3, 5, 50, 100, 150, 200}, {30, 40, 300, 32, 3, 5, 4, 8, 12, 16}};
  for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
    const int* s = bad[i];
    if (mm_co_pacrr_fwd(f, f, f, f, f, ix, 4, 1, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], NULL, 0, NULL) != MM_EUNSUPPORTED) return 10 + (int)i;
    if (mm_co_pacrr_bwd(f, f, f, ix, f, f, f, f, f, 4, 1, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], NULL, 0, NULL) != MM_EUNSUPPORTED) return 30 + (int)i;
  }
  /* workspace arithmetic is host-only: Q 4k (4 + 9) window cosines + D E + 4 E floats per pair */
  if (mm_co_pacrr_workspace_bytes(64, 30, 200, 300, 32, 3, 5) != (size_t)64 * (30 * 20 * 13 + 200 * 300 + 4 * 300) * 4) return 50;
  if (mm_co_pacrr_workspace_bytes(64, 30, 200, 300, 32, 1, 5) != (size_t)64 * (200 * 300 + 4 * 300) * 4) return 51;
  /* the backward refuses a missing workspace before any launch */
  if (mm_co_pacrr_bwd(f, f, f, ix, f, f, f, f, f, 4, 1, 30, 200, 300, 32, 3, 5, 50, 100, 150, 200, NULL, 0, NULL) != MM_EWORKSPACE) return 52;
  printf("co_pacrr c client ok: %s\n", mm_last_error());
  return 0;
}
""", name="co_pacrr_client")
    assert "co_pacrr c client ok" in out
