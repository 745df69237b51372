"""Generates tests/golden/drmm_*.npz by running the REAL DRMM class (matchmaker/models/drmm.py, imported read-only through
oracle/ref_harness.py) on seeded synthetic inputs.  Run in the build container only:

    python tests/golden/gen_golden_drmm.py

drmm.py imports allennlp's get_text_field_mask, DotProductMatrixAttention, FeedForward and Activation.  allennlp is not
installed: the first two are never called and are stubbed, FeedForward / Activation.by_name are restated here from the
published 2.x source (Linear -> activation -> Dropout(0) per layer), in this process only.  The word embedder is a module
that returns the vectors handed in beside `tokens`.  Each file holds the tokens, the vectors, the module's parameters, the
histogram the real forward fed to matching_classifier (before log1p, captured by wrapping torch.log1p during the call)
and the score.  `strict` cases (no planted exact matches) are generated only from seeds for which no fp64 cosine lies
within 1e-5 of a bin edge, so their histograms can be compared for equality."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness as R  # noqa: E402
from tests import drmm_reference as DR  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_FILE_BYTES = 1 << 20

# name: (B, Q, D, E, bins, document lengths, query lengths, OOV rows mid-document, planted exact matches, 3-D token layout)
CASES = {
    "ref": (2, 30, 200, 300, 10, None, None, False, False, False),
    "padded": (4, 30, 200, 64, 10, [200, 131, 77, 52], None, False, False, False),
    "oov": (3, 30, 200, 64, 10, [200, 150, 90], None, True, False, False),
    "qpad": (3, 30, 200, 64, 10, None, [30, 12, 5], False, False, False),
    "b1": (1, 30, 200, 64, 10, None, None, False, False, False),
    "d77": (3, 20, 77, 64, 10, None, None, False, False, False),
    "d300": (2, 30, 300, 48, 10, None, [30, 22], False, False, False),
    "bins7": (3, 30, 200, 64, 7, [200, 160, 33], None, False, False, False),
    "planted": (3, 30, 200, 64, 10, [200, 170, 120], [30, 25, 30], False, True, False),
    "elmo": (3, 16, 120, 64, 10, [120, 80, 41], [16, 9, 16], True, False, True),
}
STRICT_MARGIN = 1e-5


class _FeedForward(torch.nn.Module):
    """allennlp.modules.feedforward.FeedForward (2.x), restated."""

    def __init__(self, input_dim, num_layers, hidden_dims, activations, dropout=0.0):
        super().__init__()
        self._activations = torch.nn.ModuleList(activations)
        dims = [input_dim] + hidden_dims[:-1]
        self._linear_layers = torch.nn.ModuleList([torch.nn.Linear(i, o) for i, o in zip(dims, hidden_dims)])
        self._dropout = torch.nn.ModuleList([torch.nn.Dropout(p=dropout) for _ in hidden_dims])

    def forward(self, inputs):
        out = inputs
        for layer, act, drop in zip(self._linear_layers, self._activations, self._dropout):
            out = drop(act(layer(out)))
        return out


class _Activation:
    @staticmethod
    def by_name(name):
        return {"tanh": torch.nn.Tanh}[name]


class VecEmbedder(torch.nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def get_output_dim(self):
        return self.dim

    def forward(self, t):
        return t["vecs"]


def install_stubs(setitem=None):
    """setitem(name, module): how sys.modules entries are set (the tests pass monkeypatch.setitem)."""
    R.install_shims()
    put = setitem or sys.modules.__setitem__
    nn_mod, util = types.ModuleType("allennlp.nn"), types.ModuleType("allennlp.nn.util")
    util.get_text_field_mask = lambda *a, **kw: None
    nn_mod.util = util
    act = types.ModuleType("allennlp.nn.activations")
    act.Activation = _Activation
    ff = types.ModuleType("allennlp.modules.feedforward")
    ff.FeedForward = _FeedForward
    dp = types.ModuleType("allennlp.modules.matrix_attention.dot_product_matrix_attention")
    dp.DotProductMatrixAttention = torch.nn.Module
    put("allennlp.nn", nn_mod)
    put("allennlp.nn.util", util)
    put("allennlp.nn.activations", act)
    put("allennlp.modules.feedforward", ff)
    put("allennlp.modules.matrix_attention.dot_product_matrix_attention", dp)


def run_reference(m, query, document):
    """(score [B, 1], histogram [B, Q, bins]) of the real forward; the histogram is log1p's argument (:77)."""
    seen = {}
    real = torch.log1p

    def spy(x):
        seen["h"] = x.detach().clone()
        return real(x)

    torch.log1p = spy
    try:
        with torch.no_grad():
            s = m.forward(query, document)
    finally:
        torch.log1p = real
    return s, seen["h"]


def make_inputs(B, Q, D, E, lens, qlens, oov, planted, elmo, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    qt = torch.randint(2, 1000, (B, Q), generator=g)
    dt = torch.randint(2, 1000, (B, D), generator=g)
    if lens is not None:
        dt = dt * (torch.arange(D)[None] < torch.tensor(lens)[:, None])
    if qlens is not None:
        qt = qt * (torch.arange(Q)[None] < torch.tensor(qlens)[:, None])
    if oov:
        dt[:, 3::11] = torch.minimum(dt[:, 3::11], torch.ones_like(dt[:, 3::11]))       # OOV (1) where a token was real
        qt[:, 2] = torch.minimum(qt[:, 2], torch.ones_like(qt[:, 2]))
    if planted:
        for b in range(B):
            for j in range(0, D, 7):
                d[b, j] = q[b, (j + b) % Q]
    if elmo:                                   # character ids per word: a word is padding when its ids sum to 0
        qt = torch.stack([qt, qt * 2, qt + (qt > 1).long()], dim=-1) * (qt > 1).long().unsqueeze(-1)
        dt = torch.stack([dt, dt * 2, dt + (dt > 1).long()], dim=-1) * (dt > 1).long().unsqueeze(-1)
    return q, d, qt, dt


def masks(qt, dt):
    if qt.dim() == 2:
        return (qt > 1).float(), (dt > 1).float()
    return (qt.sum(2) > 0).float(), (dt.sum(2) > 0).float()


def gen_case(name, B, Q, D, E, bins, lens, qlens, oov, planted, elmo, seed):
    install_stubs()
    from matchmaker.models.drmm import DRMM
    strict = not planted
    while True:
        q, d, qt, dt = make_inputs(B, Q, D, E, lens, qlens, oov, planted, elmo, seed)
        qm, dm = masks(qt, dt)
        if not strict:
            break
        bd = DR.bounds(q * qm.unsqueeze(-1), d * dm.unsqueeze(-1), bins, STRICT_MARGIN)
        if bd["undecided"] == 0:
            break
        seed += 1000
    torch.manual_seed(seed)
    m = DRMM(VecEmbedder(E), bins).eval()
    s, h = run_reference(m, {"tokens": qt, "vecs": q}, {"tokens": dt, "vecs": d})
    out = {"q": q.numpy(), "d": d.numpy(), "q_tokens": qt.numpy(), "d_tokens": dt.numpy(), "score": s.numpy(),
           "hist": h.numpy(), "shape": np.array([B, Q, D, E, bins]), "strict": np.array(int(strict)), "seed": np.array(seed)}
    for key, v in m.state_dict().items():
        out["param." + key] = v.numpy()
    path = os.path.join(OUT, f"drmm_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_FILE_BYTES, (path, size)
    print(f"{path}: {size} bytes, seed {seed}, strict {strict}")


def main():
    for i, (name, case) in enumerate(CASES.items()):
        gen_case(name, *case, seed=700 + i)


if __name__ == "__main__":
    main()
