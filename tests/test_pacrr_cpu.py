"""CPU tests of PACRR (no GPU): the fp64 restatement (tests/pacrr_reference.py) against the real class's goldens and, where the
reference tree exists, against live instances; the drop-in's from_config / state_dict parity; patch_matchmaker's rebinding;
the fake (meta) implementation of torch.ops.mm_native.pacrr_kmax; the C ABI's argument checks (no device needed)."""
import sys
import types

import numpy as np
import pytest
import torch

from oracle import ref_harness as R
from tests import pacrr_reference as P
from tests import util

CFG = {"pacrr_unified_query_length": 30, "pacrr_unified_document_length": 200, "pacrr_max_conv_kernel_size": 3,
       "pacrr_conv_output_size": 32, "pacrr_kmax_pooling_size": 5}       # config/train/non-bert-defaults.yaml:54-58


def _conv(g, N):
    ws = [torch.tensor(g[f"param.convolutions.{i}.1.weight"], dtype=torch.float64) for i in range(N - 1)]
    bs = [torch.tensor(g[f"param.convolutions.{i}.1.bias"], dtype=torch.float64) for i in range(N - 1)]
    return ws, bs


def _dense(g):
    return [torch.tensor(g["param." + k], dtype=torch.float64)
            for k in ("dense.weight", "dense.bias", "dense2.weight", "dense2.bias", "dense3.weight")]


def _pad_rows_of(g):
    """(document, row) pairs that are zero padding: their cosines tie exactly, so which of them a top-k keeps is a tie
    policy and their gradients are compared as a sum."""
    B, D = g["d"].shape[:2]
    lens = g["doc_len"] if "doc_len" in g else np.full(B, D)
    return np.arange(D)[None, :] >= lens[:, None]


def _restated(g, grad=True):
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    q = torch.tensor(g["q"], dtype=torch.float64, requires_grad=grad)
    d = torch.tensor(g["d"], dtype=torch.float64, requires_grad=grad)
    ws, bs = _conv(g, N)
    for t in ws + bs:
        t.requires_grad_(grad)
    pqr = P.per_query_results(q, d, ws, bs, k)
    s = P.score(pqr, *_dense(g))
    if grad:
        s.sum().backward()
    return q, d, ws, bs, pqr, s


@pytest.mark.parametrize("name", ["ref", "b1", "q1", "n1", "n4", "k1", "padded"])
def test_restatement_matches_the_real_class_goldens(name):
    g = util.load(f"pacrr_{name}.npz")
    B, Q, D, E, N, C, k = (int(x) for x in g["shape"])
    q, d, ws, bs, pqr, s = _restated(g)
    # fp32 reference vs fp64 restatement: the cosine's fp32 rounding (~1e-7 relative) carried through <= 25-tap convs
    np.testing.assert_allclose(pqr.detach().numpy(), g["per_query_results"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(s.detach().numpy(), g["score"], rtol=1e-5, atol=1e-5)
    for i in range(N - 1):
        np.testing.assert_allclose(ws[i].grad.numpy(), g[f"grad.convolutions.{i}.1.weight"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(bs[i].grad.numpy(), g[f"grad.convolutions.{i}.1.bias"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(q.grad.numpy(), g["grad_q"], rtol=1e-4, atol=1e-4)
    pad = _pad_rows_of(g)
    gd, ref_gd = d.grad.numpy(), g["grad_d"]
    np.testing.assert_allclose(gd[~pad], ref_gd[~pad], rtol=1e-4, atol=1e-4)
    if pad.any():
        for b in range(B):
            if pad[b].any():
                got, ref = gd[b][pad[b]].sum(0), ref_gd[b][pad[b]].sum(0)
                np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(ref).max())))


def _reference_class(monkeypatch):
    """The real PACRR class, imported with pacrr.py's two allennlp imports stubbed through monkeypatch (sys.modules is
    restored afterwards, so the other tests see the module state they see without this file)."""
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
    monkeypatch.delitem(sys.modules, "matchmaker.models.pacrr", raising=False)
    import importlib
    return importlib.import_module("matchmaker.models.pacrr").PACRR


@pytest.mark.skipif(not R.available(), reason="live parity needs the reference tree; the goldens cover the rest")
@pytest.mark.parametrize("Q, D, E, N, C, k", [(30, 200, 64, 3, 32, 5), (7, 40, 24, 4, 8, 3), (12, 60, 32, 1, 16, 2)])
def test_restatement_matches_the_live_class_forward_and_autograd(monkeypatch, Q, D, E, N, C, k):
    Ref = _reference_class(monkeypatch)
    torch.manual_seed(Q + D)
    m = Ref(unified_query_length=Q, unified_document_length=D, max_conv_kernel_size=N, conv_output_size=C,
            kmax_pooling_size=k).double()
    B = 3
    q = torch.randn(B, Q, E, dtype=torch.float64, requires_grad=True)
    d = torch.randn(B, D, E, dtype=torch.float64, requires_grad=True)
    s = m(q, d, torch.ones(B, Q), torch.ones(B, D), torch.ones(B, Q, 1), torch.ones(B, D, 1))
    s.sum().backward()
    q2 = q.detach().clone().requires_grad_(True)
    d2 = d.detach().clone().requires_grad_(True)
    ws = [c[1].weight.detach().clone().requires_grad_(True) for c in m.convolutions]
    bs = [c[1].bias.detach().clone().requires_grad_(True) for c in m.convolutions]
    s2 = P.score(P.per_query_results(q2, d2, ws, bs, k), m.dense.weight, m.dense.bias, m.dense2.weight, m.dense2.bias,
                 m.dense3.weight)
    s2.sum().backward()
    torch.testing.assert_close(s2, s, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(q2.grad, q.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(d2.grad, d.grad, rtol=1e-10, atol=1e-10)
    for w, b, c in zip(ws, bs, m.convolutions):
        torch.testing.assert_close(w.grad, c[1].weight.grad, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(b.grad, c[1].bias.grad, rtol=1e-10, atol=1e-10)


def test_from_config_and_state_dict_match_the_real_class(monkeypatch):
    from matchmaker_amd.pacrr import PACRR
    mine = PACRR.from_config(CFG, 300)
    g = util.load("pacrr_ref.npz")
    keys = sorted(k[len("param."):] for k in g if k.startswith("param."))
    assert sorted(mine.state_dict()) == keys
    # the golden's real-class state_dict (Q = 30, N = 3, C = 32, k = 5, as CFG) loads strictly
    sd = {k: torch.tensor(g["param." + k]) for k in keys}
    assert all(tuple(mine.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    mine.load_state_dict(sd, strict=True)
    assert [type(c[i]).__name__ for c in mine.convolutions for i in range(3)] == ["ConstantPad2d", "Conv2d", "MaxPool3d"] * 2
    if R.available():
        Ref = _reference_class(monkeypatch)
        ref = Ref.from_config(CFG, 300)
        assert {k: v.shape for k, v in ref.state_dict().items()} == {k: v.shape for k, v in mine.state_dict().items()}
        assert sorted(n for n, _ in ref.named_parameters()) == sorted(n for n, _ in mine.named_parameters())
        mine.load_state_dict(ref.state_dict(), strict=True)
        ref.load_state_dict(mine.state_dict(), strict=True)


def test_patch_matchmaker_rebinds_pacrr(monkeypatch):
    """on the real module where the reference tree is present, on a stand-in with the same name otherwise"""
    from matchmaker_amd import patch
    from matchmaker_amd.pacrr import PACRR
    assert ("matchmaker.models.pacrr", "PACRR", "matchmaker_amd.pacrr", "PACRR") in patch._TABLE
    if R.available():
        Ref = _reference_class(monkeypatch)
        ref_mod = sys.modules["matchmaker.models.pacrr"]
        all_mod = types.ModuleType("matchmaker.models.all")
    else:
        for name in ("matchmaker", "matchmaker.models", "matchmaker.models.published"):
            monkeypatch.setitem(sys.modules, name, sys.modules.get(name) or types.ModuleType(name))
        ref_mod = types.ModuleType("matchmaker.models.pacrr")
        Ref = type("PACRR", (), {})
        ref_mod.PACRR = Ref
        monkeypatch.setitem(sys.modules, "matchmaker.models.pacrr", ref_mod)
        all_mod = types.ModuleType("matchmaker.models.all")
    all_mod.PACRR = Ref
    monkeypatch.setitem(sys.modules, "matchmaker.models.all", all_mod)
    import importlib
    for mod_name, attr, _, _ in patch._TABLE:           # every rebinding is undone afterwards: other tests drive the real classes
        try:
            mod = importlib.import_module(mod_name)
        except Exception:
            continue
        monkeypatch.setattr(mod, attr, getattr(mod, attr))
    monkeypatch.setattr(patch, "_idcm_note_given", True)
    done = patch.patch_matchmaker()
    assert "matchmaker.models.pacrr.PACRR" in done
    assert ref_mod.PACRR is PACRR and all_mod.PACRR is PACRR
    m = all_mod.PACRR.from_config(CFG, 300)             # models/all.py:159-160
    assert type(m).__module__ == "matchmaker_amd.pacrr"


@pytest.mark.parametrize("nq, ppq, B, N", [(4, 1, 4, 3), (2, 1000, 1500, 3), (3, 1, 3, 1), (1, 1, 1, 5)])
def test_fake_tensor_shapes_of_the_torch_op(nq, ppq, B, N):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from matchmaker_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        q = torch.empty(nq, 30, 300, device="cuda")
        d = torch.empty(B, 200, 300, device="cuda")
        ws = [torch.empty(32, 1, n, n, device="cuda") for n in range(2, N + 1)]
        bs = [torch.empty(32, device="cuda") for _ in range(2, N + 1)]
        out, idx = torch.ops.mm_native.pacrr_kmax(q, d, ws, bs, 5, ppq)
        assert tuple(out.shape) == (B, 30, 5 * N) and out.dtype == torch.float32
        assert tuple(idx.shape) == (B, 30, 5 * N) and idx.dtype == torch.int32
        gq, gd, gw, gb = torch.ops.mm_native.pacrr_kmax_backward(q, d, ws, idx, out, 5, ppq)
        assert tuple(gq.shape) == tuple(q.shape) and tuple(gd.shape) == tuple(d.shape)
        assert [tuple(t.shape) for t in gw] == [tuple(w.shape) for w in ws] and [tuple(t.shape) for t in gb] == [(32,)] * (N - 1)


def test_autograd_rule_shapes_on_meta_tensors():
    from matchmaker_amd import torch_ops  # noqa: F401
    q = torch.empty(2, 30, 64, device="meta", requires_grad=True)
    d = torch.empty(4, 200, 64, device="meta", requires_grad=True)
    ws = [torch.empty(32, 1, n, n, device="meta", requires_grad=True) for n in (2, 3)]
    bs = [torch.empty(32, device="meta", requires_grad=True) for _ in (2, 3)]
    for ppq in (2, 1):            # 1 = the default of the host operator: the autograd rule must not depend on it
        out, idx = torch.ops.mm_native.pacrr_kmax(q, d[:2 * ppq], ws, bs, 5, ppq)
        out.sum().backward()
    assert q.grad.shape == q.shape and d.grad.shape == d.shape
    assert [w.grad.shape for w in ws] == [w.shape for w in ws] and [b.grad.shape for b in bs] == [b.shape for b in bs]


def test_ops_reject_cpu_tensors_and_out_of_limit_shapes():
    from matchmaker_amd import ops, NativeError
    q, d = torch.zeros(1, 4, 16), torch.zeros(1, 10, 16)
    with pytest.raises(NativeError):
        ops.pacrr_kmax(q, d, [], [], 5)


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
  if (mm_pacrr_fwd(NULL, f, f, f, f, NULL, 4, 1, 30, 200, 300, 32, 3, 5, NULL, 0, NULL) != MM_EINVAL) return 1;
  if (mm_pacrr_fwd(f, f, NULL, f, f, NULL, 4, 1, 30, 200, 300, 32, 3, 5, NULL, 0, NULL) != MM_EINVAL) return 2;
  if (mm_pacrr_bwd(f, f, f, NULL, f, f, f, f, f, 4, 1, 30, 200, 300, 32, 3, 5, NULL, 0, NULL) != MM_EINVAL) return 3;
  if (mm_pacrr_bwd(f, f, f, ix, f, NULL, f, f, f, 4, 1, 30, 200, 300, 32, 3, 5, NULL, 0, NULL) != MM_EINVAL) return 4;
  if (strlen(mm_last_error()) == 0) return 5;
  /* outside the limits (pointers are host memory: nothing may be launched) */
  const int bad[][6] = {{65, 200, 300, 32, 3, 5}, {30, 4, 300, 32, 3, 5}, {30, 2049, 300, 32, 3, 5}, {30, 200, 1028, 32, 3, 5},
                        {30, 200, 302, 32, 3, 5}, {30, 200, 300, 65, 3, 5}, {30, 200, 300, 32, 6, 5}, {30, 200, 300, 32, 3, 33},
                        {30, 200, 300, 32, 0, 5}, {30, 200, 300, 32, 3, 0}, {0, 200, 300, 32, 3, 5}, {30, 200, 300, 0, 3, 5}};
  for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
    const int* s = bad[i];
    if (mm_pacrr_fwd(f, f, f, f, f, ix, 4, 1, s[0], s[1], s[2], s[3], s[4], s[5], NULL, 0, NULL) != MM_EUNSUPPORTED) return 10 + (int)i;
    if (mm_pacrr_bwd(f, f, f, ix, f, f, f, f, f, 4, 1, s[0], s[1], s[2], s[3], s[4], s[5], NULL, 0, NULL) != MM_EUNSUPPORTED) return 30 + (int)i;
  }
  /* workspace arithmetic is host-only: Q k (4 + 9) floats per pair at the reference config, none for N = 1 */
  if (mm_pacrr_workspace_bytes(64, 30, 200, 32, 3, 5) != (size_t)64 * 30 * 5 * 13 * 4) return 50;
  if (mm_pacrr_workspace_bytes(64, 30, 200, 32, 1, 5) != 0) return 51;
  /* the backward refuses a missing workspace before any launch */
  if (mm_pacrr_bwd(f, f, f, ix, f, f, f, f, f, 4, 1, 30, 200, 300, 32, 3, 5, NULL, 0, NULL) != MM_EWORKSPACE) return 52;
  printf("pacrr c client ok: %s\n", mm_last_error());
  return 0;
}
""", name="pacrr_client")
    assert "pacrr c client ok" in out
