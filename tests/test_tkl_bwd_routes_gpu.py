"""mm_tkl_bwd on every kernel its dispatch can reach and on both launch forms, against float64 gradients.

The host entry (matchmaker_amd/csrc/tkl_bwd.hip) picks tkl_bwd_tiled_kernel<5> (E <= 320), tkl_bwd_tiled_kernel<8> (E <= 512
while the tiles fit 150 KiB of LDS) or the per-element tkl_bwd_kernel (everything else, or MM_KP_BWD_UNTILED=1), and runs the
tiled kernels with three workgroups per document (3 B <= the device's CUs) or with one (larger batches, the smaller workspace,
or MM_TKL_BWD_NOSPLIT=1).  The reference is tests/tkl_bwd_cases.reference64 — autograd through the torch restatement in float64
on the CPU — at the bound the project holds this backward to (rtol 2e-3, atol 3e-4 max(1, |want|max)); chunk rows that no
selected window reads must hold exact zeros; two calls give the same bits.

The environment switches are read once per process, so the other launch form and the other kernel run in fresh children
(the _child pattern of tests/test_zz_rank_order_gpu.py: subprocess.run of a function of this module, one at a time)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import tkl_bwd_cases as T
from tests import util

pytestmark = pytest.mark.gpu

SATS = ["embedding", "log"]
ROUTES = {"nosplit": "MM_TKL_BWD_NOSPLIT", "untiled": "MM_KP_BWD_UNTILED"}
_TENSORS = ("q_ctx", "chunks", "cmask", "slot", "qm", "go")


def _native(c, dev, win=None):
    """ops.tkl_bwd on the case `c` (CPU tensors) -> (grad_q, grad_chunks, packed grad_params, win), twice: the same bits."""
    from matchmaker_amd import ops
    q_ctx, chunks, cmask, slot, qm, go = (c[k].to(dev) for k in _TENSORS)
    params = c["model"].pack_params().to(dev)
    if win is None:
        _, win = ops.tkl_score(q_ctx, chunks, cmask, slot, qm, params, c["B"], c["C"], T.K, c["sat"], return_windows=True)
    else:
        win = win.to(dev)
    out = ops.tkl_bwd(q_ctx, chunks, cmask, slot, qm, params, win, go, c["B"], c["C"], T.K, c["sat"])
    again = ops.tkl_bwd(q_ctx, chunks, cmask, slot, qm, params, win, go, c["B"], c["C"], T.K, c["sat"])
    for a, b, n in zip(out, again, ("grad_q", "grad_chunks", "grad_params")):
        assert torch.equal(a, b), f"{n}: a second call gives other bits"
    return out[0].cpu(), out[1].cpu(), out[2].cpu(), win.cpu()


def _check(label, c, win, got, ref=None):
    """The gradients `got` of case `c` against float64 at the bound, the exact zeros; prints and returns the largest ratio."""
    gq, gc, gp = got
    gq64, gc64, gp64 = ref if ref is not None else T.reference64(c["model"], c["q_ctx"], c["chunks"], c["cmask"], c["slot"], c["qm"],
                                                                 win, c["C"], c["go"])
    E = c["q_ctx"].shape[-1]
    named = T.named_from_packed(gp, c["sat"], E)
    worst = 0.0
    for n, g, w in [("grad_q", gq, gq64), ("grad_chunks", gc, gc64)] + [(n, named[n], gp64[n]) for n in gp64]:
        r = T.error_ratio(g, w)
        print(f"[tkl bwd] {label} {n}: |want|max {float(w.abs().max()) if w.numel() else 0.0:.3e} error/bound {r:.4f}")
        assert r <= 1.0, f"{label} {n}: error / bound = {r:.3f} against float64"
        worst = max(worst, r)
    print(f"[tkl bwd] {label} WORST {worst:.4f}")
    zero = T.structural_zero_rows(win, c["slot"], c["C"])
    assert (gc[zero] == 0).all(), f"{label}: grad_chunks rows outside the selected windows must be exact zeros"
    assert float(gc.abs().max()) > 0 and float(gq.abs().max()) > 0
    mu_sigma = gp[:2 * T.K]
    assert (mu_sigma == 0).all(), f"{label}: mu / sigma are not trained"
    return worst


def _splits(c):
    """Does mm_tkl_bwd give this batch three workgroups per document?  (The larger workspace is only asked for when it does.)"""
    from matchmaker_amd import _lib
    L = _lib.lib()
    Qn, En = c["q_ctx"].shape[1], c["q_ctx"].shape[2]
    return L.mm_tkl_bwd_workspace_bytes2(c["B"], c["C"], Qn, En) > L.mm_tkl_bwd_workspace_bytes(c["B"], c["C"])


def _no_switch():
    assert not any(os.environ.get(v) for v in ROUTES.values()), "the parent runs the default dispatch"


# ---- every kernel, default dispatch, natural window scores ---------------------------------------------------------------------
@pytest.mark.parametrize("sat", SATS)
@pytest.mark.parametrize("shape,kernel", T.NATURAL, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s, _ in T.NATURAL])
def test_every_kernel_of_the_default_dispatch_against_float64(shape, kernel, sat):
    """B = 3 ragged documents, window scores from mm_tkl_fwd.  E <= 320 -> tiled<5>; 320 < E <= 512 -> tiled<8>; E > 512 -> the
    per-element kernel.  (32, 120, 512) also reaches the per-element kernel: at Q = 32, E = 512, W = 46 the tiled kernel's LDS
    formula gives 188,416 bytes, above its 150 KiB limit (153,600); (12, 160, 512) needs 131,936 and stays tiled."""
    dev = util.require_gpu()
    _no_switch()
    c = T.natural(*shape, sat)
    assert _splits(c)
    gq, gc, gp, win = _native(c, dev)
    assert float((win != 0).sum()) > 0
    _check(f"{kernel}{'' if kernel == 'per-element' else ' 3wg'} {shape} {sat}", c, win, (gq, gc, gp))


@pytest.mark.parametrize("sat", SATS)
def test_one_document_above_the_split_bound_takes_one_workgroup_per_document(sat):
    """3 B > the device's CUs by default dispatch alone: every document's three regions in one workgroup."""
    dev = util.require_gpu()
    _no_switch()
    B = torch.cuda.get_device_properties(dev).multi_processor_count // 3 + 1
    c = T.natural(12, 120, 64, sat, B=B)
    assert not _splits(c)
    c1 = T.natural(12, 120, 64, sat, B=B - 1)
    assert _splits(c1), "one document fewer still takes three workgroups per document"
    gq, gc, gp, win = _native(c, dev)
    _check(f"tiled<5> 1wg B={B} {sat}", c, win, (gq, gc, gp))


# ---- the planted cases on every launch form -----------------------------------------------------------------------------------
def _planted_results(dev):
    return {(name, sat): _native(T.planted(name, sat), dev, T.planted(name, sat)["win"])[:3] for name in T.CASES for sat in SATS}


@functools.lru_cache(maxsize=None)
def _parent_results(path):
    _no_switch()
    res = _planted_results(util.require_gpu())
    np.savez(path, **{f"{name}-{sat}-{i}": g.numpy() for (name, sat), got in res.items() for i, g in enumerate(got)})
    return res


@pytest.mark.parametrize("sat", SATS)
@pytest.mark.parametrize("name", list(T.CASES))
def test_planted_regions_with_three_workgroups_per_document(name, sat, tmp_path_factory):
    res = _parent_results(str(tmp_path_factory.getbasetemp() / "tkl_bwd_parent.npz"))
    c = T.planted(name, sat)
    assert _splits(c)
    _check(f"tiled<5> 3wg {name} {sat}", c, c["win"], res[(name, sat)], T.planted_reference(name, sat))


def run_route(route, parent_npz):
    """In the child (the switch of `route` is in its environment): every planted case and every natural shape the switch
    re-routes, against float64; the planted cases against the parent's gradients as well."""
    dev = util.require_gpu()
    assert os.environ.get(ROUTES[route]) == "1" and not any(os.environ.get(v) for k, v in ROUTES.items() if k != route)
    parent = np.load(parent_npz)
    differs = 0
    for (name, sat), got in _planted_results(dev).items():
        c = T.planted(name, sat)
        assert not _splits(c) or route == "untiled"
        kernel = "tiled<5> 1wg" if route == "nosplit" else "per-element"
        _check(f"{kernel} {name} {sat}", c, c["win"], got, T.planted_reference(name, sat))
        gq_a, gc_a, gp_a = (torch.from_numpy(parent[f"{name}-{sat}-{i}"]) for i in range(3))
        dq = float((got[0] - gq_a).abs().max()) / max(float(gq_a.abs().max()), 1.0)
        dp = float((got[2] - gp_a).abs().max()) / max(float(gp_a.abs().max()), 1.0)
        dc = float((got[1] - gc_a).abs().max()) / max(float(gc_a.abs().max()), 1.0)
        print(f"[tkl bwd] {route} vs three workgroups, {name} {sat}: grad_q {dq:.3e} grad_params {dp:.3e} grad_chunks {dc:.3e} (x scale)")
        assert dq <= 2e-6 and dp <= 2e-6, (name, sat, dq, dp)
        if route == "nosplit":
            # a region's rows are one workgroup's work either way, in the same region order
            assert torch.equal(got[1], gc_a), f"{name} {sat}: grad_chunks differs from the three-workgroup launch"
        else:
            differs += int(not torch.equal(got[0], gq_a))
    if route == "untiled":
        assert differs > 0, "the per-element kernel gave the tiled kernel's bits in every case: did the switch arrive?"
    for shape, kernel in T.NATURAL:
        if kernel == "per-element":
            continue                       # (the parent ran these on the per-element kernel already, one workgroup per document)
        for sat in SATS:
            c = T.natural(*shape, sat)
            gq, gc, gp, win = _native(c, dev)
            _check(f"{kernel + ' 1wg' if route == 'nosplit' else 'per-element'} {shape} {sat}", c, win, (gq, gc, gp))
    print(f"route {route}: ok")


@pytest.mark.parametrize("route", list(ROUTES))
def test_planted_regions_with_one_workgroup_per_document_and_on_the_per_element_kernel(route, tmp_path_factory):
    """One fresh child per switch (never an exec of this process): MM_TKL_BWD_NOSPLIT=1 -> the tiled kernel with one workgroup
    per document, grad_chunks bit-equal to the three-workgroup launch; MM_KP_BWD_UNTILED=1 -> the per-element kernel at the
    same shapes.  Either child: grad_q and grad_params within 2e-6 x max(scale, 1) of the three-workgroup launch (the bound of
    test_backward_with_three_workgroups_per_document_equals_the_one_workgroup_launch; measured: <= 7.9e-7 for one workgroup,
    <= 1.7e-6 on the per-element kernel; both kernels are deterministic), and every gradient against float64."""
    path = str(tmp_path_factory.getbasetemp() / "tkl_bwd_parent.npz")
    _parent_results(path)
    env = {k: v for k, v in os.environ.items() if k not in ROUTES.values()}
    env[ROUTES[route]] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", f"from tests.test_tkl_bwd_routes_gpu import run_route; run_route({route!r}, {path!r})"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"route {route}: ok" in r.stdout


# ---- refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Qn,Kn", [(33, 11), (12, 7), (12, 12)])
def test_unsupported_shapes_are_refused_and_the_outputs_left_untouched(Qn, Kn):
    """Q > 32 query tokens and K != 11 kernels: MM_EUNSUPPORTED before any launch — grad_q, grad_chunks and grad_params as they
    were — and ops.tkl_bwd raises NativeError with that code."""
    from matchmaker_amd import _lib, ops
    dev = util.require_gpu()
    c = T.natural(Qn, 120, 64, "embedding")
    B, C, E = c["B"], c["C"], 64
    q_ctx, chunks, cmask, slot, qm, go = (c[k].to(dev) for k in _TENSORS)
    slot = slot.to(torch.int32)
    params = c["model"].pack_params().to(dev)
    P, W = chunks.shape[0], (C * 40 - 30) // 2 + 1
    win = torch.rand(B, W, device=dev) + 0.5
    L = _lib.lib()
    wsb = L.mm_tkl_bwd_workspace_bytes2(B, C, min(Qn, 32), E)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    poison = 0x7FC0BEEF                                            # (a NaN when read as float32)
    outs = [torch.full((n,), poison, dtype=torch.int32, device=dev) for n in (B * Qn * E, P * 50 * E, B * params.numel())]
    rc = L.mm_tkl_bwd(q_ctx.data_ptr(), chunks.data_ptr(), cmask.data_ptr(), slot.data_ptr(), qm.data_ptr(), params.data_ptr(),
                      win.data_ptr(), go.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), B, P, C, Qn, E, Kn, 0,
                      ws.data_ptr(), wsb, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.MM_EUNSUPPORTED, (rc, L.mm_last_error())
    for o in outs:
        assert bool((o == poison).all())
    assert not bool(ws.any()), "the workspace is untouched too"
    with pytest.raises(ops.NativeError) as e:
        ops.tkl_bwd(q_ctx, chunks, cmask, slot, qm, params, win, go, B, C, Kn, "embedding")
    assert e.value.code == _lib.MM_EUNSUPPORTED and ("Q=33" in str(e.value) if Qn == 33 else f"K={Kn}" in str(e.value))
