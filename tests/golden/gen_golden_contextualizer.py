#!/usr/bin/env python
"""Generates tests/golden/contextualizer_tk.npz by driving the REAL reference class ECAI20_TK
(matchmaker/models/published/ecai20_tk.py) through oracle/ref_harness.py's shims on CPU fp32 tensors: tk.yaml's encoder
(E 300, 10 heads, 2 layers, ff 300, hybrid mix, different positional encodings), parameters from
tests.util.set_deterministic_params, and forward_representation (:133-143) of a query batch [3, 7, 300] and a document batch
[3, 33, 300] with sequence lengths 33, 20 and 1.  Data only.  Needs the reference tree (oracle.ref_harness.REFERENCE_ROOT), so
it runs in the build container only; the tests read the file.

    python tests/golden/gen_golden_contextualizer.py

Arrays: q_emb [3, 7, 300], q_mask [3, 7], q_out [3, 7, 300], d_emb [3, 33, 300], d_mask [3, 33], d_out [3, 33, 300], float32.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from tests import util  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
E, HEADS, LAYERS, FF, MAX_LENGTH = 300, 10, 2, 300, 200      # config/train/models/tk.yaml
Q_LEN, D_LEN = (7, 4, 1), (33, 20, 1)


def make_reference_tk():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # nested tensors need batch_first: the warning the constructor gives
        m = ref_harness.make_tk(embsize=E, bypass_contextualizer=False, att_heads=HEADS, att_layer=LAYERS, att_ff_dim=FF,
                                max_length=MAX_LENGTH)
    return util.set_deterministic_params(m).eval()


def inputs():
    rng = np.random.default_rng(25)
    out = {}
    for side, lens in (("q", Q_LEN), ("d", D_LEN)):
        L = max(lens)
        mask = (np.arange(L)[None, :] < np.asarray(lens)[:, None]).astype(np.float32)
        out[side + "_emb"] = (rng.standard_normal((len(lens), L, E)) * mask[:, :, None]).astype(np.float32)      # padding embeds to 0
        out[side + "_mask"] = mask
    return out


def main():
    m = make_reference_tk()
    d = inputs()
    with torch.no_grad():
        for side, pos in (("q", m.positional_features_q), ("d", m.positional_features_d)):
            emb, mask = torch.from_numpy(d[side + "_emb"]), torch.from_numpy(d[side + "_mask"])
            d[side + "_out"] = m.forward_representation(emb, mask, pos[:, :emb.shape[1], :]).numpy()
    path = os.path.join(OUT, "contextualizer_tk.npz")
    np.savez(path, **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
