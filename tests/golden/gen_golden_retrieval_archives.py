"""Generates tests/golden/retrieval_archive_*: one saved IVF, graph and scann index over 64 vectors of dim 128 and the
(scores, ids) each returned for 4 queries at top_n 5, written by the code of the commit the script is run at (the CPU
stand-ins of the test-suite in place of the device operators).  tests/test_retrieval_base_cpu.py loads the archives with
the current code: they pin the file formats, so run this only when a format changes on purpose:

    python tests/golden/gen_golden_retrieval_archives.py

Vector and query coordinates are small integers: every inner product is exact in fp32 and no result depends on a
summation order.  IVF probes all of its 4 lists, scann searches all of its 8 leaves and re-scores every row, so the choice
of probes cannot matter either.  The data come from the first seed under which no query has two equal scores among its best 6."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import graph_reference as GR  # noqa: E402
from tests import scann_reference as SR  # noqa: E402
from tests import test_ivf_cpu as IV  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
N, E, NQ, TOP_N = 64, 128, 4, 5
CONFIGS = {
    "ivf": {"token_dim": E, "faiss_ivf_list_count": 4, "faiss_ivf_search_probe_count": 4},
    "graph": {"token_dim": E, "faiss_hnsw_graph_neighbors": 8, "faiss_hnsw_efSearch": 64},
    "scann": {"token_dim": E, "token_dtype": "float16", "scann_leaves_to_search": 8, "scann_reorder": 64},
}


def indexer(kind):
    from matchmaker_amd import retrieval as RT
    if kind == "ivf":
        return RT.IVFFlatIPIndexer(CONFIGS[kind], device="cpu", topk_fn=IV._topk_fn, scan_fn=IV._scan_fn, merge_fn=IV._merge_fn)
    if kind == "graph":
        return RT.GraphIPIndexer(CONFIGS[kind], device="cpu", topk_fn=GR.topk_fn, search_fn=GR.search_fn, merge_fn=GR.merge_fn)
    return RT.ScannIPIndexer(CONFIGS[kind], device="cpu", topk_fn=SR.topk_fn, encode_fn=SR.encode_fn, scan_fn=SR.scan_fn,
                             rescore_fn=SR.rescore_fn, merge_fn=SR.merge_fn)


def archive(kind):
    return os.path.join(OUT, "retrieval_archive_" + kind + ("" if kind == "scann" else ".npz"))


def main():
    for seed in range(100):                                    # the first seed whose queries have no tie among their best
        rng = np.random.default_rng(seed)
        x = rng.integers(-3, 4, (N, E)).astype(np.float32)
        q = rng.integers(-3, 4, (NQ, E)).astype(np.float32)
        exact = np.sort(q @ x.T, axis=1)[:, ::-1][:, : TOP_N + 1]
        if (np.diff(exact, axis=1) < 0).all():
            break
    else:
        raise SystemExit("two equal scores among a query's best under every seed")
    ids = np.arange(N, dtype=np.int64) * 3 + 5
    expected = {"queries": q}
    for kind in CONFIGS:
        ix = indexer(kind)
        ix.prepare([x[:20], x[20:]])
        ix.index([ids[:20], ids[20:]], [x[:20], x[20:]])
        ix.save(archive(kind))
        s, i = ix.search(q, TOP_N)
        assert (np.diff(s, axis=1) < 0).all() and (i >= 0).all(), kind
        expected[kind + "_scores"], expected[kind + "_ids"] = s, i
        print(kind, i.tolist())
    np.savez(os.path.join(OUT, "retrieval_archive_expected.npz"), **expected)


if __name__ == "__main__":
    main()
