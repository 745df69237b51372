"""CPU: the TK-Sparse and IDCM-sampler restatements (oracle/np_oracle.py, oracle/torch_port.py) against golden
vectors of the real classes (tests/golden/gen_golden.py: gen_tk_sparse, gen_idcm), and the host logic of the
IDCM drop-in (windowing, selection, top-k combination) with the oracle standing in for the native operator —
tests may use the oracle; the product path has no CPU fallback (asserted at the end)."""
import numpy as np
import pytest
import torch

from tests.tkl_window_reference import selected_window_scores

from oracle import np_oracle as O
from oracle import torch_port as TP
from tests import util

MU = [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9]
SIGMA = [0.1] * 11


def _params(g):
    return {k[len("param."):]: v for k, v in g.items() if k.startswith("param.")}


def test_tk_sparse_oracle_matches_reference_golden():
    g = util.load("sparse_tk_q20_d200_e300.npz")
    p = _params(g)
    q, d, qm, dm = g["q"], g["d"], g["q_mask"], g["d_mask"]
    # the gate as the reference's MLP makes it (:132-133; bypassed contextualiser: both mix inputs are d)
    h = np.tanh(d @ p["stop_word_reducer.weight"].T + p["stop_word_reducer.bias"])
    gate = np.maximum(h @ p["stop_word_reducer2.weight"].T + p["stop_word_reducer2.bias"], 0)[..., 0] * dm
    np.testing.assert_allclose(gate, g["document_stop_words"][:, 0], atol=2e-5)
    assert 0.2 < (gate[0] == 0).mean() < 0.8, "the fixture must exercise closed and open gates"
    qin, din = q * qm[..., None], d * dm[..., None]                # forward_representation's mask multiply (:170)
    for dtype, tol in ((np.float32, 3e-4), (np.float64, 3e-4)):
        s, pk = O.tk_sparse_kernel_pool(qin, din, qm, dm, g["document_stop_words"][:, 0], MU, SIGMA,
                                        p["kernel_alpha_scaler"].reshape(-1), p["kernel_bin_weights.weight"].reshape(-1),
                                        dtype=dtype, return_per_kernel=True)
        np.testing.assert_allclose(pk, g["per_kernel"], atol=tol, rtol=2e-5)
        np.testing.assert_allclose(s, g["score"], atol=tol, rtol=2e-5)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).float()
    st = TP.tk_sparse_kernel_pool(t(qin), t(din), t(qm), t(dm), t(g["document_stop_words"]),
                                  torch.tensor(MU).view(1, 1, 1, -1), torch.tensor(SIGMA).view(1, 1, 1, -1),
                                  t(p["kernel_alpha_scaler"]), t(p["kernel_bin_weights.weight"]))
    np.testing.assert_allclose(st.numpy(), g["score"], atol=3e-4, rtol=2e-5)


def test_gate_is_tk_with_weighted_document_mask():
    """The scoring block of TK-Sparse equals TK's with the {0,1} document mask replaced by mask x gate: the
    identity the native kernel relies on (cosine masking before the kernels, :114, changes no pooled sum)."""
    rng = np.random.default_rng(5)
    B, Q, D, E = 3, 7, 19, 16
    q, d = rng.standard_normal((B, Q, E)).astype(np.float32), rng.standard_normal((B, D, E)).astype(np.float32)
    qm = (np.arange(Q)[None] < np.array([7, 3, 1])[:, None]).astype(np.float32)
    dm = (np.arange(D)[None] < np.array([19, 4, 11])[:, None]).astype(np.float32)
    gate = np.maximum(rng.standard_normal((B, D)), 0).astype(np.float32) * dm
    alpha, w = rng.random(11).astype(np.float32) + 0.5, rng.standard_normal(11).astype(np.float32)
    a = O.tk_sparse_kernel_pool(q, d, qm, dm, gate, MU, SIGMA, alpha, w, dtype=np.float64)
    b = O.tk_kernel_pool(q, d, qm, gate, MU, SIGMA, alpha, w, dtype=np.float64)       # gate in the mask's place
    np.testing.assert_allclose(a, b, atol=1e-9)


def _tiny_distilbert():
    from transformers import DistilBertConfig, DistilBertModel
    cfg = DistilBertConfig(vocab_size=200, dim=64, n_heads=4, hidden_dim=128, n_layers=2,
                           max_position_embeddings=128, dropout=0.0, attention_dropout=0.0)
    return DistilBertModel(cfg).eval()


def _oracle_kernel_pool(q, d, q_mask, d_mask, mu, sigma, alpha, w, clamp_min=1e-10, pair_query=None, **kw):
    assert clamp_min == 1e-4 and kw.get("d_gate") is None
    if pair_query is not None:                             # ragged groups: the query row of each passage
        q, q_mask = q[pair_query.long()], q_mask[pair_query.long()]
    n = lambda t: t.detach().cpu().numpy()
    s = O.idcm_sampler_scores(n(q), n(d), n(q_mask), n(d_mask), n(mu).reshape(-1), n(sigma).reshape(-1),
                              n(alpha).reshape(-1), n(w).reshape(-1), 0.0)
    s = torch.from_numpy(s.astype(np.float32))
    return (s, None) if kw.get("return_pooled") else s      # (the training node asks for the pooled sums; the stand-in has none)


@pytest.mark.parametrize("fname,ctx_kind", [("idcm_ck.npz", "ck"), ("idcm_ck_small.npz", "ck-small")])
def test_idcm_host_logic_and_sampler_oracle_match_reference_golden(monkeypatch, fname, ctx_kind):
    from matchmaker_amd import ops
    from tests import idcm_host_fixture as idcm
    g = util.load(fname)
    m = idcm.IDCM(_tiny_distilbert(), sample_n=2, sample_context=ctx_kind, top_k_chunks=2, chunk_size=50, overlap=7,
                  padding_idx=0, sample_train_type="mseloss")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _params(g).items()}, strict=True)
    m.eval()
    monkeypatch.setattr(ops, "kernel_pool", _oracle_kernel_pool)
    t = lambda k: torch.from_numpy(g[k])
    with torch.no_grad():
        score, bert_scores, sec, _, _ = m.forward({"input_ids": t("q_ids"), "attention_mask": t("q_mask")},
                                                  {"input_ids": t("d_ids"), "attention_mask": t("d_mask")},
                                                  use_fp16=False, output_secondary_output=True)
        plain = m.forward({"input_ids": t("q_ids"), "attention_mask": t("q_mask")},
                          {"input_ids": t("d_ids"), "attention_mask": t("d_mask")}, use_fp16=False)
    assert (sec["packed_indices"].numpy() == g["packed_indices"]).all()
    np.testing.assert_allclose(sec["sampling_scores"].numpy(), g["sampling_scores"], atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(bert_scores.numpy(), g["bert_scores"], atol=1e-5)
    np.testing.assert_allclose(score.numpy(), g["score"], atol=1e-5)
    # the cached-BERT path (re-ranking with stored passage scores) reproduces the same document score
    with torch.no_grad():
        cached = m.forward({"input_ids": t("q_ids"), "attention_mask": t("q_mask")},
                           {"input_ids": t("d_ids"), "attention_mask": t("d_mask")}, use_fp16=False,
                           output_secondary_output=True, bert_part_cached=torch.from_numpy(g["bert_scores"]).clone())[0]
    np.testing.assert_allclose(cached.numpy(), g["score"], atol=1e-5)
    # training mode without the secondary output: (score, passage scores, [[loss]], orders)
    m.train()
    out = m.forward({"input_ids": t("q_ids"), "attention_mask": t("q_mask")},
                    {"input_ids": t("d_ids"), "attention_mask": t("d_mask")}, use_fp16=False)
    assert len(out) == 4 and out[2][0][0].dim() == 0 and out[3][0].shape == g["packed_indices"].shape
    assert isinstance(plain, tuple) and len(plain) == 4      # eval without secondary output takes the same branch


def test_variant_operators_have_no_cpu_fallback():
    from matchmaker_amd import ops
    q, d = torch.zeros(1, 4, 8), torch.zeros(1, 5, 8)
    z = torch.zeros(11)
    with pytest.raises(ops.NativeError):
        ops.kernel_pool(q, d, None, None, z, z + 0.1, z + 1, z, d_gate=torch.ones(1, 5), clamp_min=1e-4)


# ---- TKL training path: the selected-window gradient carrier vs gradients of the real class ---------------------

def _tkl_bypass(E, sat, params):
    from matchmaker_amd.tkl import TKL_sigir20

    class Bypass(TKL_sigir20):   # mirrors oracle/ref_harness.TKLBypass
        def forward_representation(self, emb, mask, positional_features=None):
            return emb * mask.unsqueeze(-1), emb

    m = Bypass(E, MU, SIGMA, 8, 1, 32, 2000, True, True, sat)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=False)
    assert not unexpected and all(k.startswith(("contextualizer", "positional")) for k in missing)
    return m


def check_tkl_grads(m, g, q, d, tol=2e-4):
    for name, got in (("grad_q", q.grad), ("grad_d", d.grad)):
        want = g[name]
        np.testing.assert_allclose(got.detach().cpu().numpy(), want, atol=tol * max(1.0, np.abs(want).max()), rtol=2e-3,
                                   err_msg=name)
    n = 0
    for k, p in m.named_parameters():
        if "grad." + k in g:
            want = g["grad." + k]
            assert p.grad is not None, k
            np.testing.assert_allclose(p.grad.detach().cpu().numpy(), want, atol=tol * max(1.0, np.abs(want).max()),
                                       rtol=2e-3, err_msg=k)
            n += 1
    assert n >= 3


def test_tkl_gradient_carrier_matches_gradients_of_the_real_class():
    """grad_tkl_*.npz: gradients of the REAL TKL_sigir20.forward.  The carrier (tests/tkl_window_reference.selected_window_scores) is pure
    torch, so it runs on the CPU here, fed with the fixture's window scores in place of the native ones."""
    from matchmaker_amd.tkl import chunk_documents
    g = util.load("grad_tkl_d333_e64_embedding.npz")
    m = _tkl_bypass(64, "embedding", _params(g)).train()
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k])).float()
    q, d = t("q").requires_grad_(True), t("d").requires_grad_(True)
    q_ctx, _ = m.forward_representation(q, t("q_mask"))
    chunks, chunk_mask, chunk_slot, C = chunk_documents(d, t("d_mask"))
    chunks_ctx, _ = m.forward_representation(chunks, chunk_mask)
    s = selected_window_scores(m, q_ctx, chunks_ctx, chunk_mask, chunk_slot, t("q_mask"), t("orig_score"), C)
    np.testing.assert_allclose(s.detach().numpy(), g["score"], atol=1e-4, rtol=1e-5)
    (s * t("grad_out")).sum().backward()
    check_tkl_grads(m, g, q, d)


def _idcm_case(case, ctx_kind, sample_n, seed):
    """(drop-in, REAL class or None, inputs, recorded outputs) of one tests/golden/idcm_live.npz case: both models get the
    parameters of tests/util.set_deterministic_params, so the real class's recorded outputs hold for the drop-in too; the
    real class is built live where the reference tree is present"""
    from oracle import ref_harness as R
    from tests import idcm_host_fixture as idcm
    g = {k[len(case) + 1:]: v for k, v in util.load("idcm_live.npz").items() if k.startswith(case + ".")}
    mine = idcm.IDCM(_tiny_distilbert(), sample_n=sample_n, sample_context=ctx_kind, top_k_chunks=3, chunk_size=50, overlap=7,
                     padding_idx=0, sample_train_type="mseloss")
    util.set_deterministic_params(mine).eval()
    assert sorted(mine.state_dict().keys()) == g["state_dict_keys"].tolist()
    ref = None
    if R.available():
        ref = util.set_deterministic_params(R.make_idcm(_tiny_distilbert(), sample_n=sample_n, sample_context=ctx_kind,
                                                        top_k_chunks=3, seed=seed))
        mine.load_state_dict(ref.state_dict(), strict=True)
    t = lambda k: torch.from_numpy(g[k]).long()
    query = {"input_ids": t("q_ids"), "attention_mask": t("q_mask")}
    doc = {"input_ids": t("d_ids"), "attention_mask": t("d_mask")}
    return mine, ref, query, doc, g


@pytest.mark.parametrize("ctx_kind", ["tk", "ck", "ck-small"])
def test_idcm_dropin_equals_the_live_reference_class_for_every_sampler(monkeypatch, ctx_kind):
    """No weights fixture for the "tk" sampler (its Transformer weights are 3.5 MB): the REAL IDCM's outputs are recorded
    with parameters derived from their names (tests/golden/idcm_live.npz), or it runs live next to the drop-in where the
    reference tree is present (CPU, oracle in the native operator's place)."""
    from matchmaker_amd import ops
    monkeypatch.setattr(ops, "kernel_pool", _oracle_kernel_pool)
    mine, ref, query, doc, g = _idcm_case(ctx_kind.replace("-", "_"), ctx_kind, 3, 5)
    with torch.no_grad():
        if ref is not None:
            want = ref.forward(query, doc, use_fp16=False, output_secondary_output=True)
            want = (want[0].numpy(), want[1].numpy(), want[2]["sampling_scores"].numpy())
        else:
            want = (g["score"], g["scores_1"], g["sampling_scores"])
        got = mine.forward(query, doc, use_fp16=False, output_secondary_output=True)
    np.testing.assert_allclose(got[2]["sampling_scores"].numpy(), want[2], atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(got[1].numpy(), want[1], atol=1e-5)
    np.testing.assert_allclose(got[0].numpy(), want[0], atol=1e-5)


def test_idcm_without_sampling_equals_the_live_reference_class():
    """idcm.yaml's default is idcm_sample_n: -1 — no passage selection, BERT reads every packed passage
    (sigir21_idcm.py:209-252); the branch never touches the native operator, so it runs on the CPU as is.  The REAL
    class's outputs: recorded (tests/golden/idcm_live.npz) or live, as above."""
    mine, ref, query, doc, g = _idcm_case("no_sampling", "ck", -1, 6)
    with torch.no_grad():
        if ref is not None:
            want, wsec = ref.forward(query, doc, use_fp16=False, output_secondary_output=True)
            want, bert_scores, packed = want.numpy(), wsec["bert_scores"].numpy(), wsec["packed_indices"].numpy()
        else:
            want, bert_scores, packed = g["score"], g["bert_scores"], g["packed_indices"]
        got, gsec = mine.forward(query, doc, use_fp16=False, output_secondary_output=True)
        plain = mine.forward(query, doc, use_fp16=False)
    np.testing.assert_allclose(got.numpy(), want, atol=1e-5)
    np.testing.assert_allclose(gsec["bert_scores"].numpy(), bert_scores, atol=1e-5)
    assert (gsec["packed_indices"].numpy() == packed).all() and torch.equal(plain, got)
    # training: gradients reach BERT (the grad-enabled branch of :213)
    mine.train()
    mine.forward(query, doc, use_fp16=False).sum().backward()
    assert mine._classification_layer.weight.grad.abs().sum() > 0


@pytest.mark.skipif(not __import__("oracle.ref_harness", fromlist=["available"]).available(),
                    reason="the maintainer-side edit is applied to the reference tree's own source")
def test_the_maintainer_side_idcm_edit_of_integration_md_reproduces_the_real_class(monkeypatch):
    """IDCM's forward is out of scope and the product does not restate it: patch_matchmaker() leaves IDCM alone, and
    INTEGRATION.md shows the edit a maintainer makes at sigir21_idcm.py:182-186.  Here that edit is APPLIED — to the source
    text of the reference's module, in memory — and the edited class is compared with the untouched one on the same
    state_dict and inputs (CPU: the oracle stands in the operator's place)."""
    import importlib
    import types
    from oracle import ref_harness as R
    from matchmaker_amd import ops, patch
    R.install_shims()
    assert not any(ref_attr == "IDCM" for _, ref_attr, _, _ in patch._TABLE)
    import matchmaker_amd.idcm as product
    assert not hasattr(product, "forward_native") and not hasattr(product, "native_subclass")
    ref_mod = importlib.import_module("matchmaker.models.published.sigir21_idcm")
    real = ref_mod.IDCM
    src = open(ref_mod.__file__).read()
    lines = src.split("\n")
    # :182-186 = the bmm, the kernel activations, the log pooling and the bin weights (1-based, inclusive)
    block = "\n".join(lines[181:186])
    assert "torch.bmm(query_ctx" in lines[181] and "packed_patch_scores = self.sampling_binweights" in lines[185], block
    indent = lines[181][:len(lines[181]) - len(lines[181].lstrip())]
    edit = [indent + "from matchmaker_amd.idcm import sampler_scores",
            indent + "packed_patch_scores = sampler_scores(query_ctx, document_ctx, packed_query_mask, mask_packed, self.mu, self.sigma,",
            indent + "                                     self.kernel_alpha_scaler, self.sampling_binweights)"]
    edited = types.ModuleType("sigir21_idcm_with_the_maintainer_edit")
    edited.__file__ = ref_mod.__file__
    exec(compile("\n".join(lines[:181] + edit + lines[186:]), ref_mod.__file__ + " (+ INTEGRATION.md edit)", "exec"), edited.__dict__)
    torch.manual_seed(5)
    mine = edited.IDCM(_tiny_distilbert(), sample_train_type="mseloss", sample_n=3, sample_context="ck-small", top_k_chunks=3,
                       chunk_size=50, overlap=7, padding_idx=0)          # the reference's constructor (:27-108)
    ref = real(_tiny_distilbert(), sample_train_type="mseloss", sample_n=3, sample_context="ck-small", top_k_chunks=3,
               chunk_size=50, overlap=7, padding_idx=0)
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine.eval(), ref.eval()
    monkeypatch.setattr(ops, "kernel_pool", _oracle_kernel_pool)
    g = torch.Generator().manual_seed(3)
    B, LQ, LD = 3, 10, 260
    q_mask = (torch.arange(LQ)[None] < torch.tensor([10, 4, 7])[:, None]).long()
    d_mask = (torch.arange(LD)[None] < torch.tensor([260, 33, 150])[:, None]).long()
    query = {"input_ids": torch.randint(1, 200, (B, LQ), generator=g) * q_mask, "attention_mask": q_mask}
    doc = {"input_ids": torch.randint(1, 200, (B, LD), generator=g) * d_mask, "attention_mask": d_mask}
    with torch.no_grad():
        want = ref.forward(query, doc, use_fp16=False, output_secondary_output=True)
        got = mine.forward(query, doc, use_fp16=False, output_secondary_output=True)
    np.testing.assert_allclose(got[2]["sampling_scores"].numpy(), want[2]["sampling_scores"].numpy(), atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(got[0].numpy(), want[0].numpy(), atol=1e-5)
    # patch_matchmaker() rebinds the in-scope classes and leaves IDCM the reference's own
    saved = {}
    for ref_m, ref_attr, _, _ in patch._TABLE:
        try:
            saved[(ref_m, ref_attr)] = getattr(importlib.import_module(ref_m), ref_attr)
        except Exception:
            pass
    try:
        done = patch.patch_matchmaker()
        assert "matchmaker.models.published.sigir21_idcm.IDCM" not in done and ref_mod.IDCM is real
    finally:                                             # other tests drive the real classes
        for (ref_m, ref_attr), obj in saved.items():
            setattr(importlib.import_module(ref_m), ref_attr, obj)


def test_rbf_recurrence_arithmetic_stays_within_rounding_of_the_exact_kernels():
    """The pooling epilogue evaluates the reference's ten equally spaced kernels (knrm.py:33-50 kernel_mus / kernel_sigmas;
    ecai20_tk.py:47-50) by recurrence from the two middle ones (kp_device.h rbf_geo_one).  Its fp32 arithmetic, emulated
    operation for operation, against the exact kernel values over the whole cosine range: never more than 1e-5 relative on
    any activation that matters (> 1e-6), i.e. within 3 x the direct form's own rounding and a tenth of what the split-bf16
    cosine contributes; masked positions (cosine 1e5) give exact zeros; other kernel sets are refused."""
    from oracle import np_oracle as O
    mu = [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9]
    sg = [0.001] + [0.1] * 10
    c = np.linspace(-1.0, 1.0, 400001).astype(np.float32)
    geo = O.rbf_recurrence_fp32(c, mu, sg)
    direct = O.rbf_direct_fp32(c, mu, sg)
    assert geo is not None
    c64 = c.astype(np.float64)
    worst_geo = worst_direct = 0.0
    for k in range(11):
        true = np.exp(-(c64 - mu[k]) ** 2 / (2 * float(np.float32(sg[k])) ** 2))
        m = true > 1e-6
        if not m.any():
            continue
        worst_geo = max(worst_geo, float((np.abs(geo[m, k] - true[m]) / true[m]).max())) if k else worst_geo
        worst_direct = max(worst_direct, float((np.abs(direct[m, k] - true[m]) / true[m]).max())) if k else worst_direct
        if k == 0:      # the exact-match kernel is the direct form in both
            assert np.array_equal(geo[:, 0], direct[:, 0])
    assert worst_geo < 1.0e-5, worst_geo
    assert worst_geo < 3.0 * worst_direct, (worst_geo, worst_direct)
    # masked positions: exactly zero in every kernel
    assert not O.rbf_recurrence_fp32(np.array([1.0e5, -1.0e5], np.float32), mu, sg).any()
    # sets the device keeps on the direct form
    assert O.rbf_recurrence_fp32(c[:4], mu[:4] + [0.35] + mu[5:], sg) is None
    assert O.rbf_recurrence_fp32(c[:4], mu, sg[:6] + [0.15] + sg[7:]) is None
    assert O.rbf_recurrence_fp32(c[:4], [1.0] + mu[:0:-1], sg) is None
    assert O.rbf_recurrence_fp32(c[:4], mu, [0.001] + [0.04] * 10) is None
    assert O.rbf_recurrence_fp32(c[:4], [1.0] + [m + 0.5 for m in mu[1:]], sg) is None
