"""The eight mm_*_workspace_bytes of the retrieval family against tests/golden/retrieval_workspace_sizes.json, the answers of the
last commit that summed every layout by hand beside the pointer walk of its entry point
(tests/golden/gen_golden_retrieval_workspace_sizes.py).  Each size is now what the operator's one layout function leaves in a
measuring cursor (matchmaker_amd/csrc/launch_geometry.h): it has to be the same number for every shape.  Pure host code:
nothing touches a device."""
import json
import os

import pytest

from tests.golden import gen_golden_retrieval_workspace_sizes as G

with open(G.OUT) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def L():
    from matchmaker_amd import _lib, build
    build.build()
    return _lib.lib()


def test_the_file_holds_the_generators_grids():
    """... so a shape added to a grid without regenerating (or a query dropped from the file) fails here, not silently."""
    assert {name: [r["args"] for r in rows] for name, rows in GOLDEN.items()} == G.GRIDS
    assert len(GOLDEN) == 8


@pytest.mark.parametrize("name", sorted(G.GRIDS))
def test_size_query_answers_what_it_answered(L, name):
    fn = getattr(L, name)
    got = [int(fn(*r["args"])) for r in GOLDEN[name]]
    bad = [(r["args"], r["bytes"], g) for r, g in zip(GOLDEN[name], got) if g != r["bytes"]]
    assert not bad, bad[:5]


def test_the_grids_cross_the_branches_they_name():
    """What the generator's comments promise, read off the recorded answers."""
    sizes = {name: {tuple(r["args"]): r["bytes"] for r in rows} for name, rows in GOLDEN.items()}
    for name, rows in sizes.items():
        assert 0 in rows.values() and max(rows.values()) > 0, name                  # refusals and answers
    g = sizes["mm_graph_search_workspace_bytes"]
    assert 256 in g.values() and max(g.values()) > 256                              # visited table in LDS / in global memory
    for name in ("mm_ivf_scan_workspace_bytes", "mm_ivf_scan_fp8_workspace_bytes", "mm_ah_scan_workspace_bytes"):
        ivf = sizes[name]
        assert ivf == sizes["mm_ivf_scan_workspace_bytes"]                          # one layout serves the three scans
        cap = lambda n: max(1 << 28, 2 * n)                                         # noqa: E731
        one = [a for a in ivf if min(a[:4]) > 0 and a[2] * a[0] <= cap(a[0])]
        many = [a for a in ivf if min(a[:4]) > 0 and a[2] * a[0] > cap(a[0])]
        assert one and len(many) >= 8
        # several rounds: the candidate buffer stops growing with the queries (it holds cap floats, not nq * n)
        assert all(ivf[a] < 4 * cap(a[0]) + (1 << 28) for a in many)
    assert sizes["mm_dot_topk_workspace_bytes"] == sizes["mm_dot_topk_fp8_workspace_bytes"]
