"""Generates tests/golden/retrieval_workspace_sizes.json: what the eight mm_*_workspace_bytes of the retrieval family answer,
shape by shape, in the library of the commit the script is run at (pure host code: no device is touched).
tests/test_retrieval_workspace_sizes_cpu.py asks the current library the same questions: the file pins the sizes across
changes of how the layouts are written down (it was written at the last commit that summed them by hand), so run this only
when a layout changes on purpose:

    python tests/golden/gen_golden_retrieval_workspace_sizes.py        (MM_NATIVE_LIB=... for another build of the library)

The grids cross every branch of the size arithmetic; each list below says which."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "retrieval_workspace_sizes.json")


def _product(*axes):
    return [list(t) for t in itertools.product(*axes)]


# (n_docs, nq, k).  n_docs: 4096 / 4097 = "everything is a candidate" (capacity 4096) on and off, 16384 = the sample size
# (S = min(n_docs, 16384)); nq: 128 / 129 = one / two query tiles per wavefront; k: 4 k below, at and above the capacity floor
# of 1024 (256 -> 1024, 1000 -> 4096).  Then the shapes that answer 0.
DOT = _product((1, 4096, 4097, 16383, 16384, 16385, 8841823), (1, 128, 129, 6980), (1, 10, 256, 1000)) + \
    [[0, 4, 10], [-1, 4, 10], [100, 0, 10], [100, -3, 10], [100, 4, 0], [100, 4, -1]]

# (n, nlist, nq, nprobe, k).  One round while nq * n <= max(2^28, 2 n), several above: 300 x 1,000,000 and 6,980 x 1,000,000
# cross 2^28; 3 x 100,000,000 crosses it while 2 x 100,000,000 = 2 n does not, and 3 x 200,000,000 has 2 n above 2^28.
# n = 0 is a valid (empty) store; k does not enter the size.
IVF = _product((0, 1, 40, 2000, 1000000), (1, 8, 2500), (1, 3, 64, 300, 6980), (1, 4096), (10,)) + \
    _product((100000000, 200000000), (1, 2500), (1, 2, 3, 64), (1, 4096), (1, 4096)) + \
    [[-1, 8, 3, 2, 10], [40, 0, 3, 2, 10], [40, -1, 3, 2, 10], [40, 8, 0, 2, 10], [40, 8, -2, 2, 10], [40, 8, 3, 0, 10],
     [40, 8, 3, -1, 10]]

# (n, nlist, E).  n / 512 chunks + one per list; n = 0 is valid.
KMEANS = _product((0, 40, 511, 512, 5000, 1100000), (1, 3, 65536), (128, 768)) + \
    [[-1, 3, 128], [40, 0, 128], [40, -1, 128], [40, 3, 0], [40, 3, -128]]

# (n, nq, M, ef, width, n_entry, max_iters).  The visited table is in LDS (answer 256) while 2 * (n_entry + max_iters * width * M)
# fits, else one slice per workgroup (at most 1024) of pow2(2 * min(bound, n)) slots, 64 at least.  Then the envelope's refusals.
GRAPH = [[40, 3, 4, 8, 2, 2, 12], [20000, 64, 32, 64, 4, 8, 24], [20000, 64, 32, 64, 4, 8, 64], [20000, 5000, 32, 64, 4, 8, 64],
         [20, 3, 32, 64, 4, 8, 64], [1000000, 1, 128, 2048, 8, 1, 65536], [100, 7, 2, 1, 1, 1, 1],
         [0, 3, 4, 8, 2, 2, 12], [40, 0, 4, 8, 2, 2, 12], [40, 3, 3, 8, 2, 2, 12], [40, 3, 130, 8, 2, 2, 12], [40, 3, 4, 0, 2, 2, 12],
         [40, 3, 4, 4096, 2, 2, 12], [40, 3, 4, 8, 0, 2, 12], [40, 3, 4, 8, 9, 2, 12], [40, 3, 4, 8, 2, 0, 12], [40, 3, 4, 8, 2, 9, 12],
         [40, 3, 4, 8, 2, 2, 0], [40, 3, 4, 8, 2, 2, 65537]]

# (nq, H).  One slice of pow2(H) keys per workgroup, at most 1024 workgroups; H outside 1 .. 16384 answers 0.
COLBERT = _product((1, 3, 5000), (1, 8, 512, 16384)) + _product((1023, 1024, 1025), (5, 4097)) + \
    [[0, 8], [-1, 8], [3, 0], [3, -1], [3, 16385]]

GRIDS = {
    "mm_dot_topk_workspace_bytes": DOT,
    "mm_dot_topk_fp8_workspace_bytes": DOT,
    "mm_ivf_scan_workspace_bytes": IVF,
    "mm_ivf_scan_fp8_workspace_bytes": IVF,
    "mm_ah_scan_workspace_bytes": IVF,
    "mm_graph_search_workspace_bytes": GRAPH,
    "mm_kmeans_segment_sum_workspace_bytes": KMEANS,
    "mm_colbert_candidates_workspace_bytes": COLBERT,
}


def main():
    from matchmaker_amd import _lib
    L = _lib.lib()
    out = {name: [{"args": args, "bytes": int(getattr(L, name)(*args))} for args in grid] for name, grid in GRIDS.items()}
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": [\n  ' + ",\n  ".join(json.dumps(r) for r in rows) + "\n ]"
                                  for name, rows in out.items()) + "\n}\n")
    print(_lib.LIB_PATH, {name: len(rows) for name, rows in out.items()})


if __name__ == "__main__":
    main()
