"""Generates tests/golden/matchpyramid_*.npz by running the REAL MatchPyramid class (matchmaker/models/matchpyramid.py,
imported read-only through oracle/ref_harness.py) on seeded synthetic inputs.  Run in the build container only:

    python tests/golden/gen_golden_matchpyramid.py

matchpyramid.py imports allennlp.nn.util.get_text_field_mask and DotProductMatrixAttention, which the hot path never calls:
both are stubbed here (in this process only).  Each file holds the inputs, the module's parameters (`param.*`), `features`
(the input of `dense`, captured by a forward hook), `score`, `pool0` (layer 0's pooled output), `pools` and `shape`.
E <= 64 keeps every file under 1 MiB."""
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
DEFAULT = ([16] * 5, [[3, 3]] * 5, [[36, 90], [18, 60], [9, 30], [6, 20], [3, 10]])

# name: (B, Q, D, E, (channels, kernels, pools), document lengths or None, hot)
CASES = {
    "ref": (3, 30, 200, 64, DEFAULT, None, False),
    "b1": (1, 30, 200, 48, DEFAULT, None, False),
    "padded": (4, 30, 200, 64, DEFAULT, [200, 131, 77, 52], False),
    "up": (2, 5, 7, 16, ([3, 4], [[3, 3], [3, 3]], [[7, 4], [2, 3]]), None, False),
    "one": (2, 1, 2, 8, ([2], [[3, 3]], [[1, 1]]), None, False),
    "rect": (2, 6, 9, 8, ([3, 2], [[2, 3], [3, 2]], [[4, 5], [2, 2]]), None, False),
    "chan": (2, 12, 40, 32, ([5, 20, 32], [[1, 1], [5, 5], [2, 2]], [[6, 20], [4, 9], [2, 3]]), None, False),
    "hot": (2, 30, 200, 64, DEFAULT, None, True),
}


def install_stubs(setitem=None):
    """setitem(name, module): how sys.modules entries are added (a test passes monkeypatch.setitem to undo them)"""
    R.install_shims()
    put = setitem or sys.modules.__setitem__
    if "allennlp.nn.util" not in sys.modules:
        nn_mod = types.ModuleType("allennlp.nn")
        util = types.ModuleType("allennlp.nn.util")
        util.get_text_field_mask = lambda *a, **kw: None
        nn_mod.util = util
        put("allennlp.nn", nn_mod)
        put("allennlp.nn.util", util)
    dp = sys.modules["allennlp.modules.matrix_attention.dot_product_matrix_attention"]
    if not hasattr(dp, "DotProductMatrixAttention"):
        dp.DotProductMatrixAttention = torch.nn.Module


def make_reference(pyramid, seed):
    install_stubs()
    from matchmaker.models.matchpyramid import MatchPyramid
    torch.manual_seed(seed)
    channels, kernels, pools = pyramid
    return MatchPyramid(conv_output_size=channels, conv_kernel_size=kernels, adaptive_pooling_size=pools).eval()


def run_reference(m, q, d):
    """(score [B], features [B, F] = the dense layer's input, pool0 = layer 0's pooled output) of the real forward"""
    seen = {}
    h1 = m.dense.register_forward_hook(lambda mod, inp, out: seen.__setitem__("x", inp[0]))
    h2 = getattr(m.conv_layers, "pool 0").register_forward_hook(lambda mod, inp, out: seen.__setitem__("p0", out))
    B = q.shape[0]
    try:
        with torch.no_grad():
            s = m.forward(q, d, torch.ones(B, q.shape[1]), torch.ones(B, d.shape[1]))
    finally:
        h1.remove()
        h2.remove()
    return s, seen["x"], seen["p0"]


def make_inputs(B, Q, D, E, lens, seed):
    g = torch.Generator().manual_seed(seed + 1)
    q = torch.randn(B, Q, E, generator=g)
    d = torch.randn(B, D, E, generator=g)
    if lens is not None:
        d = d * (torch.arange(D)[None, :, None] < torch.tensor(lens)[:, None, None]).float()
    return q, d


def gen_case(name, B, Q, D, E, pyramid, lens, hot, seed):
    m = make_reference(pyramid, seed)
    q, d = make_inputs(B, Q, D, E, lens, seed)
    if hot:
        # default-initialised deep layers shrink under ReLU: scale every conv weight by one constant, doubled until the
        # final features reach magnitude 1
        scale = 1.0
        base = {k: v.clone() for k, v in m.state_dict().items()}
        while True:
            with torch.no_grad():
                for k, v in m.state_dict().items():
                    if k.startswith("conv_layers.") and k.endswith(".weight"):
                        v.copy_(base[k] * scale)
            if float(run_reference(m, q, d)[1].abs().max()) >= 1.0:
                break
            scale *= 2.0
        print(f"hot: conv weights scaled by {scale}")
    s, feat, p0 = run_reference(m, q, d)
    out = {"q": q.numpy(), "d": d.numpy(), "score": s.numpy(), "features": feat.numpy(), "pool0": p0.numpy(),
           "pools": np.array(pyramid[2]), "shape": np.array([B, Q, D, E, len(pyramid[0])])}
    if lens is not None:
        out["doc_len"] = np.array(lens)
    for key, v in m.state_dict().items():
        out["param." + key] = v.numpy()
    path = os.path.join(OUT, f"matchpyramid_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_FILE_BYTES, (path, size)
    zero = float((feat == 0).float().mean())
    print(f"{path}: {size} bytes, max |features| = {float(feat.abs().max()):.3e}, zero share = {zero:.2f}")


def main():
    for i, (name, case) in enumerate(CASES.items()):
        gen_case(name, *case, seed=700 + i)


if __name__ == "__main__":
    main()
