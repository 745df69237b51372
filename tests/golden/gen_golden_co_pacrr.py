"""Generates tests/golden/co_pacrr_*.npz by running the REAL CO_PACRR class (matchmaker/models/co_pacrr.py, imported
read-only through oracle/ref_harness.py) on seeded synthetic inputs.  Run in the build container only:

    python tests/golden/gen_golden_co_pacrr.py

co_pacrr.py imports allennlp.nn.util.get_text_field_mask and DotProductMatrixAttention, which the hot path never calls: both
are stubbed here (in this process only).  Each file holds the inputs, the module's parameters, per_query_results (the dense
layer's input, :168), the score, and the gradients of score.sum() w.r.t. q, d and the conv weights / biases.  E <= 64 keeps
every file under 1 MiB; the first dense layer's weights (8 k N Q x 100) are rounded to a 2^-8 grid for the same reason."""
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

# name: (B, Q, U, D, E, N, C, k, document lengths or None, query lengths or None)
CASES = {
    "ref": (3, 30, 200, 200, 64, 3, 32, 5, None, None),
    "short": (3, 30, 200, 37, 64, 3, 32, 5, None, None),        # D < v_0 = 50
    "mid": (3, 30, 200, 120, 60, 3, 32, 5, None, None),         # v_1 < D < v_2
    "long": (2, 30, 200, 260, 48, 3, 32, 5, None, None),        # D > U: halo and context windows past U
    "oddu": (3, 20, 30, 30, 64, 3, 16, 5, None, None),          # views 7 / 15 / 22 / 30
    "padded": (4, 30, 200, 200, 48, 3, 32, 5, [200, 131, 77, 52], None),
    "qpad": (3, 30, 200, 200, 48, 3, 32, 5, None, [30, 12, 5]),
    "b1": (1, 30, 200, 200, 48, 3, 32, 5, None, None),
    "n1": (3, 30, 200, 200, 64, 1, 32, 5, None, None),
    "k1": (3, 30, 200, 200, 64, 3, 32, 1, None, None),
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


def make_reference(Q, U, N, C, k, seed):
    install_stubs()
    from matchmaker.models.co_pacrr import CO_PACRR
    torch.manual_seed(seed)
    return CO_PACRR(unified_query_length=Q, unified_document_length=U, max_conv_kernel_size=N, conv_output_size=C,
                    kmax_pooling_size=k).eval()


def run_reference(m, q, d):
    """(score, per_query_results [B, Q, 8 k N]) of the real forward; per_query_results is the dense layer's input (:168)."""
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


def gen_case(name, B, Q, U, D, E, N, C, k, lens, qlens, seed):
    m = make_reference(Q, U, N, C, k, seed)
    with torch.no_grad():     # 8k N Q x 100 weights: on a 2^-8 grid they compress, and every file stays under 1 MiB
        m.dense.weight.copy_(torch.round(m.dense.weight * 256) / 256)
    g = torch.Generator().manual_seed(seed + 1)
    q = torch.randn(B, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    if lens is not None:
        d = d * (torch.arange(D)[None, :, None] < torch.tensor(lens)[:, None, None]).float()
    if qlens is not None:
        q = q * (torch.arange(Q)[None, :, None] < torch.tensor(qlens)[:, None, None]).float()
    q.requires_grad_(True)
    d.requires_grad_(True)
    s, pqr = run_reference(m, q, d)
    s.sum().backward()
    out = {"q": q.detach().numpy(), "d": d.detach().numpy(), "score": s.detach().numpy(),
           "per_query_results": pqr.detach().numpy(), "grad_q": q.grad.numpy(), "grad_d": d.grad.numpy(),
           "shape": np.array([B, Q, D, E, N, C, k]), "U": np.array(U)}
    if lens is not None:
        out["doc_len"] = np.array(lens)
    if qlens is not None:
        out["query_len"] = np.array(qlens)
    for key, v in m.state_dict().items():
        out["param." + key] = v.numpy()
    for i, conv in enumerate(m.convolutions):
        out[f"grad.convolutions.{i}.1.weight"] = conv[1].weight.grad.numpy()
        out[f"grad.convolutions.{i}.1.bias"] = conv[1].bias.grad.numpy()
    path = os.path.join(OUT, f"co_pacrr_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_FILE_BYTES, (path, size)
    print(f"{path}: {size} bytes")


def main():
    for i, (name, case) in enumerate(CASES.items()):
        gen_case(name, *case, seed=500 + i)


if __name__ == "__main__":
    main()
