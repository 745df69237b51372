"""Generates tests/golden/pacrr_*.npz by running the REAL PACRR class (matchmaker/models/pacrr.py, imported read-only
through oracle/ref_harness.py) on seeded synthetic inputs.  Run in the build container only:

    python tests/golden/gen_golden_pacrr.py

pacrr.py imports allennlp.nn.util.get_text_field_mask and DotProductMatrixAttention, which the hot path never calls: both
are stubbed here (in this process only).  Each file holds the inputs, the module's parameters, per_query_results (the dense
layer's input, :101), the score, and the gradients of score.sum() w.r.t. q, d and the conv weights / biases.  E <= 64 keeps
every file under 1 MiB."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_FILE_BYTES = 1 << 20

# name: (B, Q, D, E, N, C, k, document lengths or None)
CASES = {
    "ref": (3, 30, 200, 64, 3, 32, 5, None),
    "b1": (1, 30, 200, 48, 3, 32, 5, None),
    "q1": (3, 1, 120, 64, 3, 32, 5, None),
    "n1": (3, 30, 200, 64, 1, 32, 5, None),
    "n4": (2, 20, 150, 64, 4, 16, 5, None),
    "k1": (3, 30, 200, 64, 3, 32, 1, None),
    "padded": (4, 30, 200, 64, 3, 32, 5, [200, 131, 77, 52]),
}


def install_stubs():
    R.install_shims()
    if "allennlp.nn.util" not in sys.modules:
        nn_mod = types.ModuleType("allennlp.nn")
        util = types.ModuleType("allennlp.nn.util")
        util.get_text_field_mask = lambda *a, **kw: None
        nn_mod.util = util
        sys.modules["allennlp.nn"] = nn_mod
        sys.modules["allennlp.nn.util"] = util
    dp = sys.modules["allennlp.modules.matrix_attention.dot_product_matrix_attention"]
    if not hasattr(dp, "DotProductMatrixAttention"):
        dp.DotProductMatrixAttention = torch.nn.Module


def make_reference(Q, D, N, C, k, seed):
    install_stubs()
    from matchmaker.models.pacrr import PACRR
    torch.manual_seed(seed)
    return PACRR(unified_query_length=Q, unified_document_length=D, max_conv_kernel_size=N, conv_output_size=C,
                 kmax_pooling_size=k)


def run_reference(m, q, d):
    """(score, per_query_results [B, Q, k N]) of the real forward; per_query_results is the dense layer's input (:101)."""
    seen = {}
    h = m.dense.register_forward_hook(lambda mod, inp, out: seen.__setitem__("x", inp[0]))
    B, Q = q.shape[0], q.shape[1]
    qm, dm = torch.ones(B, Q), torch.ones(B, d.shape[1])
    idf = torch.ones(B, Q, 1)
    try:
        s = m.forward(q, d, qm, dm, idf, torch.ones(B, d.shape[1], 1))
    finally:
        h.remove()
    return s, seen["x"].reshape(B, Q, -1)


def gen_case(name, B, Q, D, E, N, C, k, lens, seed):
    m = make_reference(Q, D, N, C, k, seed)
    g = torch.Generator().manual_seed(seed + 1)
    q = torch.randn(B, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    if lens is not None:
        d = d * (torch.arange(D)[None, :, None] < torch.tensor(lens)[:, None, None]).float()
    q.requires_grad_(True)
    d.requires_grad_(True)
    s, pqr = run_reference(m, q, d)
    s.sum().backward()
    out = {"q": q.detach().numpy(), "d": d.detach().numpy(), "score": s.detach().numpy(),
           "per_query_results": pqr.detach().numpy(), "grad_q": q.grad.numpy(), "grad_d": d.grad.numpy(),
           "shape": np.array([B, Q, D, E, N, C, k])}
    if lens is not None:
        out["doc_len"] = np.array(lens)
    for key, v in m.state_dict().items():
        out["param." + key] = v.numpy()
    for i, conv in enumerate(m.convolutions):
        out[f"grad.convolutions.{i}.1.weight"] = conv[1].weight.grad.numpy()
        out[f"grad.convolutions.{i}.1.bias"] = conv[1].bias.grad.numpy()
    path = os.path.join(OUT, f"pacrr_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_FILE_BYTES, (path, size)
    print(f"{path}: {size} bytes")


def main():
    for i, (name, case) in enumerate(CASES.items()):
        gen_case(name, *case, seed=300 + i)


if __name__ == "__main__":
    main()
