"""CPU tests of DRMM (no GPU): the fp64 restatement (tests/drmm_reference.py) against the real class's goldens and, where
the reference tree exists, against live instances; the drop-in's state_dict parity; patch_matchmaker's rebinding; the fake
(meta) implementations of torch.ops.mm_native.drmm_hist / drmm_score; the host and C ABI refusals (no device needed).

Histograms: equality on strict cases (no fp64 cosine near a bin edge), the decided-element bounds of DESIGN.md §3.9 on the
planted case, with tol = 4 x max |c32 - c64| measured per case and at most 0.5 % of the elements undecided.  Scores within
1e-5: every term is gate x tanh(.), gates sum to 1 and tanh outputs lie in (-1, 1), so the fp32 head is within a few ulp
of 1."""
import importlib
import sys
import types

import numpy as np
import pytest
import torch

from oracle import ref_harness as R
from tests import drmm_reference as DR
from tests import util

CASES = ["ref", "padded", "oov", "qpad", "b1", "d77", "d300", "bins7", "planted", "elmo"]
CAP = 0.005


def masked_inputs(g, dtype=torch.float64):
    qt, dt = torch.tensor(g["q_tokens"]), torch.tensor(g["d_tokens"])
    if qt.dim() == 2:
        qm, dm = (qt > 1), (dt > 1)
    else:
        qm, dm = (qt.sum(2) > 0), (dt.sum(2) > 0)
    q = torch.tensor(g["q"], dtype=dtype) * qm.unsqueeze(-1).to(dtype)
    d = torch.tensor(g["d"], dtype=dtype) * dm.unsqueeze(-1).to(dtype)
    return q, d, qm, dm


class VecEmbedder(torch.nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def get_output_dim(self):
        return self.dim

    def forward(self, t):
        return t["vecs"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_real_class_goldens(name):
    g = util.load(f"drmm_{name}.npz")
    B, Q, D, E, bins = (int(x) for x in g["shape"])
    q, d, qm, dm = masked_inputs(g)
    tol = DR.measured_tol(q, d)
    bd = DR.bounds(q, d, bins, tol, q_rows=qm)
    msg = f"drmm_{name}: tol = {tol:.3e}, undecided = {bd['undecided']}, share = {bd['share']:.3e}"
    print(msg)
    assert bd["share"] <= CAP, msg
    ref_hist = torch.tensor(g["hist"])
    assert tuple(ref_hist.shape) == (B, Q, bins)
    h64 = DR.histogram(q, d, bins)
    if int(g["strict"]):
        assert bd["undecided"] == 0, msg
        assert torch.equal(h64, ref_hist.double()), msg
        assert (ref_hist.sum(-1) == D).all()
        s64 = DR.score(q, d, qm.double(), DR.params64(g), bins)
        np.testing.assert_allclose(s64.numpy(), g["score"], rtol=0, atol=1e-5)
    else:
        assert bd["undecided"] > 0
        DR.check_hist(ref_hist, bd, tol, f"drmm_{name} (real class)")
        DR.check_hist(h64, bd, tol, f"drmm_{name} (restatement)")
        # the head on the real class's own histogram reproduces its score
        p = DR.params64(g)
        s = DR.head(ref_hist.double(), DR.gate(q, qm.double(), p), p)
        np.testing.assert_allclose(s.numpy(), g["score"], rtol=0, atol=1e-5)


def test_padding_and_query_padding_semantics_of_the_goldens():
    """padded document positions and OOV rows count in bin bins // 2, padded query rows put all D counts there"""
    g = util.load("drmm_qpad.npz")
    B, Q, D, E, bins = (int(x) for x in g["shape"])
    _, _, qm, _ = masked_inputs(g)
    h = torch.tensor(g["hist"])
    assert (h[~qm][:, bins // 2] == D).all() and (h[~qm].sum(-1) == D).all()
    g = util.load("drmm_padded.npz")
    _, _, _, dm = masked_inputs(g)
    h = torch.tensor(g["hist"])
    assert (h[:, :, int(g["shape"][4]) // 2] >= (~dm).sum(1)[:, None]).all()
    g = util.load("drmm_bins7.npz")                      # odd bin count: a zero cosine is mid-bin 3
    _, _, _, dm = masked_inputs(g)
    assert (torch.tensor(g["hist"])[:, :, 3] >= (~dm).sum(1)[:, None]).all()


def _reference_class(monkeypatch):
    from tests.golden import gen_golden_drmm as G
    G.install_stubs(lambda k, v: monkeypatch.setitem(sys.modules, k, v))
    monkeypatch.delitem(sys.modules, "matchmaker.models.drmm", raising=False)
    return importlib.import_module("matchmaker.models.drmm").DRMM, G


@pytest.mark.skipif(not R.available(), reason="live parity needs the reference tree; the goldens cover the rest")
@pytest.mark.parametrize("B, Q, D, E, bins", [(3, 30, 200, 64, 10), (2, 7, 45, 24, 16), (2, 12, 60, 32, 5)])
def test_restatement_matches_the_live_class(monkeypatch, B, Q, D, E, bins):
    Ref, G = _reference_class(monkeypatch)
    q, d, qt, dt = G.make_inputs(B, Q, D, E, [D, D // 2, D // 3][:B], None, True, False, False, seed=Q + D)
    torch.manual_seed(bins)
    m = Ref(VecEmbedder(E), bins).eval()
    s, h = G.run_reference(m, {"tokens": qt, "vecs": q}, {"tokens": dt, "vecs": d})
    assert tuple(s.shape) == (B, 1)
    qm, dm = (qt > 1), (dt > 1)
    q64, d64 = q.double() * qm.unsqueeze(-1), d.double() * dm.unsqueeze(-1)
    tol = DR.measured_tol(q64, d64)
    bd = DR.bounds(q64, d64, bins, tol, q_rows=qm)
    assert bd["share"] <= CAP
    DR.check_hist(h, bd, tol, "live class")
    # the fp32 restatement of the bin rule is histc itself, bit for bit, on the class's own fp32 cosine
    c32 = DR.cosine(q * qm.unsqueeze(-1), d * dm.unsqueeze(-1))
    assert torch.equal(DR.histc_rows(c32, bins), h)
    p = {k: v.double() for k, v in m.state_dict().items()}
    s64 = DR.head(h.double(), DR.gate(q64, qm.double(), p), p)
    np.testing.assert_allclose(s64.numpy(), s.numpy(), rtol=0, atol=1e-5)


def test_module_imports_without_a_gpu_and_state_dict_matches_the_real_class(monkeypatch):
    from matchmaker_amd.drmm import DRMM
    g = util.load("drmm_ref.npz")
    B, Q, D, E, bins = (int(x) for x in g["shape"])
    mine = DRMM(VecEmbedder(E), bins)
    keys = sorted(k[len("param."):] for k in g if k.startswith("param."))
    assert sorted(mine.state_dict()) == keys
    assert keys == sorted(f"{m}._linear_layers.{i}.{p}" for m in ("matching_classifier", "query_gate") for i in (0, 1)
                          for p in ("weight", "bias"))
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == {k: tuple(g["param." + k].shape) for k in keys}
    sd = {k: torch.tensor(g["param." + k]) for k in keys}
    mine.load_state_dict(sd, strict=True)
    for k, v in mine.state_dict().items():
        assert torch.equal(v, sd[k])
    assert mine.get_param_stats() == "DRMM: -" and mine.bin_count == bins
    # the torch head of the drop-in on the golden histogram gives the golden score (no GPU involved)
    q, d, qm, dm = masked_inputs(g, torch.float32)
    gates = mine.query_softmax(mine.query_gate(q).squeeze(-1), qm.float())
    s = torch.sum(mine.matching_classifier(torch.log1p(torch.tensor(g["hist"]))) * gates.unsqueeze(-1), dim=1)
    np.testing.assert_allclose(s.detach().numpy(), g["score"], rtol=0, atol=1e-5)
    if R.available():
        Ref, _ = _reference_class(monkeypatch)
        ref = Ref(VecEmbedder(E), bins)
        assert {k: v.shape for k, v in ref.state_dict().items()} == {k: v.shape for k, v in mine.state_dict().items()}
        mine.load_state_dict(ref.state_dict(), strict=True)
        ref.load_state_dict(mine.state_dict(), strict=True)


def test_masked_softmax_keeps_the_reference_edge_cases():
    from matchmaker_amd.drmm import MaskedSoftmax
    x = torch.tensor([[0.3, -0.2, 0.9], [0.1, 0.2, 0.3]])
    mask = torch.tensor([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    out = MaskedSoftmax()(x, mask)
    assert out[0, 1] == 0 and abs(float(out[0].sum()) - 1) < 1e-6
    assert torch.isnan(out[1]).all()                       # every token masked: NaN, as in the reference
    torch.testing.assert_close(out[0], DR.masked_softmax(x.double(), mask.double())[0].float())


def test_patch_matchmaker_rebinds_drmm(monkeypatch):
    """on the real module where the reference tree is present, on a stand-in with the same name otherwise"""
    from matchmaker_amd import patch
    from matchmaker_amd.drmm import DRMM
    assert ("matchmaker.models.drmm", "DRMM", "matchmaker_amd.drmm", "DRMM") in patch._TABLE
    if R.available():
        Ref, _ = _reference_class(monkeypatch)
        ref_mod = sys.modules["matchmaker.models.drmm"]
    else:
        for name in ("matchmaker", "matchmaker.models"):
            monkeypatch.setitem(sys.modules, name, sys.modules.get(name) or types.ModuleType(name))
        ref_mod = types.ModuleType("matchmaker.models.drmm")
        Ref = type("DRMM", (), {})
        ref_mod.DRMM = Ref
        monkeypatch.setitem(sys.modules, "matchmaker.models.drmm", ref_mod)
    all_mod = types.ModuleType("matchmaker.models.all")
    all_mod.DRMM = Ref
    monkeypatch.setitem(sys.modules, "matchmaker.models.all", all_mod)
    for mod_name, attr, _, _ in patch._TABLE:           # every rebinding is undone afterwards
        try:
            mod = importlib.import_module(mod_name)
        except Exception:
            continue
        monkeypatch.setattr(mod, attr, getattr(mod, attr))
    monkeypatch.setattr(patch, "_idcm_note_given", True)
    done = patch.patch_matchmaker()
    assert "matchmaker.models.drmm.DRMM" in done
    assert ref_mod.DRMM is DRMM and all_mod.DRMM is DRMM
    m = all_mod.DRMM(VecEmbedder(32), 10)               # models/all.py:154
    assert type(m).__module__ == "matchmaker_amd.drmm"


@pytest.mark.parametrize("nq, ppq, B, bins", [(4, 1, 4, 10), (2, 1000, 1500, 10), (1, 1, 1, 16), (3, 1, 3, 7)])
def test_fake_tensor_shapes_of_the_torch_ops(nq, ppq, B, bins):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from matchmaker_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        q = torch.empty(nq, 30, 300, device="cuda")
        d = torch.empty(B, 200, 300, device="cuda")
        h = torch.ops.mm_native.drmm_hist(q, d, bins, ppq)
        assert tuple(h.shape) == (B, 30, bins) and h.dtype == torch.float32
        h = torch.ops.mm_native.drmm_hist(q, d, bins, ppq, torch.empty(B, dtype=torch.int32, device="cuda"), True)
        assert tuple(h.shape) == (B, 30, bins)
        s = torch.ops.mm_native.drmm_score(q, d, torch.empty(nq, 30, device="cuda"), torch.empty(bins, bins, device="cuda"),
                                           torch.empty(bins, device="cuda"), torch.empty(1, bins, device="cuda"),
                                           torch.empty(1, device="cuda"), ppq)
        assert tuple(s.shape) == (B,) and s.dtype == torch.float32


def test_histogram_op_is_non_differentiable_and_score_op_refuses_training():
    from matchmaker_amd import torch_ops, NativeError  # noqa: F401
    q = torch.empty(2, 30, 64, device="meta", requires_grad=True)
    d = torch.empty(2, 200, 64, device="meta", requires_grad=True)
    h = torch.ops.mm_native.drmm_hist(q, d, 10, 1)
    assert not h.requires_grad
    W1 = torch.empty(10, 10, device="meta", requires_grad=True)
    s = torch.ops.mm_native.drmm_score(q.detach(), d.detach(), torch.empty(2, 30, device="meta"), W1,
                                       torch.empty(10, device="meta"), torch.empty(1, 10, device="meta"),
                                       torch.empty(1, device="meta"), 1)
    with pytest.raises(NativeError, match="inference-only"):
        s.sum().backward()


def test_ops_reject_cpu_tensors_and_out_of_limit_shapes():
    from matchmaker_amd import ops, NativeError
    q, d = torch.zeros(1, 4, 16), torch.zeros(1, 60, 16)
    with pytest.raises(NativeError):
        ops.drmm_hist(q, d)
    with pytest.raises(NativeError):
        ops.drmm_score(q, d, torch.zeros(1, 4), torch.zeros(10, 10), torch.zeros(10), torch.zeros(10), torch.zeros(1))
    for Q, D, E, bins in [(65, 200, 64, 10), (30, 65536, 64, 10), (30, 200, 1028, 10), (30, 200, 64, 17), (30, 200, 64, 0)]:
        with pytest.raises(NativeError, match="MM_EUNSUPPORTED"):
            ops._drmm_shapes(torch.empty(2, Q, E, device="meta"), torch.empty(2, D, E, device="meta"), 1, bins, "drmm_hist")
    with pytest.raises(NativeError, match="pairs"):
        ops._drmm_shapes(torch.empty(3, 30, 64, device="meta"), torch.empty(2, 200, 64, device="meta"), 1, 10, "drmm_hist")


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
  if (mm_drmm_fwd(NULL, f, NULL, f, NULL, NULL, 0, NULL, NULL, NULL, NULL, 4, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 1;
  if (mm_drmm_fwd(f, NULL, NULL, f, NULL, NULL, 0, NULL, NULL, NULL, NULL, 4, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 2;
  /* neither output */
  if (mm_drmm_fwd(f, f, ix, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, 4, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 3;
  /* score without its head parameters / gate */
  if (mm_drmm_fwd(f, f, NULL, NULL, f, NULL, 0, f, f, f, f, 4, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 4;
  if (mm_drmm_fwd(f, f, NULL, NULL, f, f, 0, f, NULL, f, f, 4, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 5;
  /* inconsistent scalars */
  if (mm_drmm_fwd(f, f, NULL, f, NULL, NULL, 0, NULL, NULL, NULL, NULL, -1, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 6;
  if (mm_drmm_fwd(f, f, NULL, f, NULL, NULL, 0, NULL, NULL, NULL, NULL, 4, 0, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 7;
  if (mm_drmm_fwd(f, f, NULL, f, NULL, NULL, 2, NULL, NULL, NULL, NULL, 4, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_EINVAL) return 8;
  if (mm_drmm_fwd(f, f, NULL, f, NULL, NULL, 0, NULL, NULL, NULL, NULL, 4, 1, 30, 200, 300, 10, 2, NULL, 0, NULL) != MM_EINVAL) return 9;
  if (strlen(mm_last_error()) == 0) return 10;
  /* outside the limits (pointers are host memory: nothing may be launched) */
  const int bad[][4] = {{65, 200, 300, 10}, {0, 200, 300, 10}, {30, 65536, 300, 10}, {30, 0, 300, 10}, {30, 200, 1028, 10},
                        {30, 200, 302, 10}, {30, 200, 0, 10}, {30, 200, 300, 17}, {30, 200, 300, 0}};
  for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
    const int* s = bad[i];
    if (mm_drmm_fwd(f, f, NULL, f, NULL, NULL, 0, NULL, NULL, NULL, NULL, 4, 1, s[0], s[1], s[2], s[3], 0, NULL, 0, NULL) != MM_EUNSUPPORTED) return 20 + (int)i;
    if (mm_drmm_fwd(f, f, ix, f, f, f, 1, f, f, f, f, 4, 1, s[0], s[1], s[2], s[3], 1, NULL, 0, NULL) != MM_EUNSUPPORTED) return 40 + (int)i;
  }
  /* no pairs: nothing to do, nothing launched */
  if (mm_drmm_fwd(f, f, NULL, f, NULL, NULL, 0, NULL, NULL, NULL, NULL, 0, 1, 30, 200, 300, 10, 0, NULL, 0, NULL) != MM_OK) return 60;
  if (mm_drmm_workspace_bytes(64000, 30, 200, 300, 10) != 0) return 61;
  if (mm_abi_version() != 4) return 62;
  printf("drmm c client ok\n");
  return 0;
}
""", name="drmm_client")
    assert "drmm c client ok" in out
