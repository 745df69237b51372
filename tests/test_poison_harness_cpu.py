"""CPU: the poisoned-memory harness (tests/poison.py) has teeth, and its case table covers the operator surface.

The harness runs here on CPU tensors against fake operators written in this file, shaped like the ones of matchmaker_amd/ops.py
(outputs from `torch.empty`, a workspace from `_workspace`, a "kernel" that fills them): one leaves an element unwritten, one
writes a byte past an output, one writes a byte past the workspace size it declared.  Each must be caught by the assertion
meant for it and by no other, and a correct one must pass.  No kernel is broken anywhere to show this.

The coverage check parses matchmaker_amd/ops.py: every public function that reaches `_call` or `_topk_reruns` (directly or
through the module's private helpers) has a case in tests/test_poisoned_memory_gpu.py or a written waiver there."""
import ast
import os
import types

import pytest
import torch

from tests import poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raw_bytes(t, nbytes_past_start):
    """`nbytes_past_start` bytes of memory from t's first byte on, t's own storage allowing (what a kernel holding t's
    pointer can reach): a uint8 view that may run past t's end."""
    st = t.untyped_storage()
    whole = torch.empty(0, dtype=torch.uint8).set_(st, 0, (st.nbytes(),))
    off = t.storage_offset() * t.element_size()
    return whole[off:off + nbytes_past_start]


def _fake_ops(skip=None, out_overrun=0, ws_overrun=0, ws_declared=64):
    """A module like ops.py with one operator: out[i] = 2 x[i] + (the sum of x, staged through the workspace)."""
    m = types.ModuleType("fake_ops")
    m.torch = torch
    m._WS = {}

    def _workspace(dev, nbytes, stream=None):      # the cached, over-sized buffer of ops._workspace
        t = m._WS.get(dev)
        if t is None or t.numel() < nbytes:
            t = m._WS[dev] = m.torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        return t

    def clear_workspaces():
        m._WS.clear()

    def scale(x):
        n = x.shape[0]
        out = m.torch.empty(n, dtype=torch.float32, device=x.device)
        ws = m._workspace(x.device, ws_declared)
        # ---- the "kernel": works on raw memory, as a HIP kernel does
        stage = _raw_bytes(ws, ws_declared + ws_overrun)
        stage[:4] = x.sum().reshape(1).view(torch.uint8)
        if ws_overrun:
            stage[ws_declared:] = 0xA5
        total = stage[:4].clone().view(torch.float32)[0]
        for i in range(n):
            if i != skip:
                out[i] = 2 * x[i] + total
        if out_overrun:
            _raw_bytes(out, n * 4 + out_overrun)[n * 4:] = 0xA5
        return out

    m._workspace, m.clear_workspaces, m.scale = _workspace, clear_workspaces, scale
    return m


X = torch.arange(1, 8, dtype=torch.float32)


def _both(m):
    return [poison.run(lambda: m.scale(X), p, module=m, label="fake") for p in poison.POISONS]


def test_correct_operator_passes():
    m = _fake_ops()
    (a, arena_a), (b, _) = _both(m)
    poison.assert_same_bits(a, b, "fake")
    assert torch.equal(a, 2 * X + X.sum())
    assert poison.poison_survivors(a, 0xFF) == 0
    # what the harness promises of every allocation: alignment, guard bands, the record, the exact workspace size
    assert len(arena_a.allocations) == 2
    out_rec, ws_rec = arena_a.allocations
    assert (out_rec.nbytes, out_rec.dtype, out_rec.shape) == (28, torch.float32, (7,))
    assert (ws_rec.nbytes, ws_rec.dtype, ws_rec.shape) == (64, torch.uint8, (64,))
    for rec in arena_a.allocations:
        assert (rec.buffer.data_ptr() + rec.offset) % poison.ALIGN == 0
        assert rec.offset >= poison.GUARD and rec.buffer.numel() - rec.offset - rec.nbytes >= poison.GUARD
    # and the module is as it was
    assert m.torch is torch and not m._WS


def test_unwritten_element_is_caught_by_the_bit_comparison():
    m = _fake_ops(skip=3)
    (a, _), (b, _) = _both(m)                      # guards intact: run() asserted them
    with pytest.raises(AssertionError, match=r"differs between the two poisons in 1 of 7 elements, first at \[3\]"):
        poison.assert_same_bits(a, b, "fake")
    assert poison.poison_survivors(a, 0xFF) == 1 and poison.poison_survivors(b, 0x7F) == 1
    # an element the header calls unspecified may be left out, and nothing more
    keep = torch.ones(7, dtype=torch.bool)
    keep[3] = False
    poison.assert_same_bits(a, b, "fake", keep=[keep])
    keep[3], keep[2] = True, False
    with pytest.raises(AssertionError):
        poison.assert_same_bits(a, b, "fake", keep=[keep])


def test_value_computed_from_uninitialised_memory_is_caught():
    m = _fake_ops()
    inner = m.scale

    def reads_before_writing(x):
        ws = m._workspace(x.device, 64)
        return inner(x) + ws[:4].clone().view(torch.float32)[0]       # reads the workspace before anything wrote it
    m.scale = reads_before_writing
    (a, _), (b, _) = _both(m)
    with pytest.raises(AssertionError, match="differs between the two poisons in 7 of 7"):
        poison.assert_same_bits(a, b, "fake")


@pytest.mark.parametrize("p", poison.POISONS)
def test_write_past_an_output_is_caught_by_its_guard(p):
    m = _fake_ops(out_overrun=1)
    with pytest.raises(AssertionError, match=r"allocation 0 \(torch.float32 \(7,\), 28 bytes\): 1 guard byte\(s\) after it"):
        poison.run(lambda: m.scale(X), p, module=m, label="fake")


@pytest.mark.parametrize("p", poison.POISONS)
def test_write_past_the_declared_workspace_is_caught_by_its_guard(p):
    m = _fake_ops(ws_overrun=1)
    with pytest.raises(AssertionError, match=r"allocation 1 \(torch.uint8 \(64,\), 64 bytes\): 1 guard byte\(s\) after it"):
        poison.run(lambda: m.scale(X), p, module=m, label="fake")
    # without the harness the cached 64 KiB workspace swallows the same overrun
    assert torch.equal(m.scale(X), 2 * X + X.sum())


def test_write_before_an_allocation_is_caught():
    with poison.poisoned(0xFF, module=_fake_ops()) as arena:
        t = arena.empty((3, 5), dtype=torch.int64)
        assert (t == -1).all()                                          # 0xFF: -1 in every integer type
        arena.allocations[0].buffer[arena.allocations[0].offset - 1] = 0
    assert "1 guard byte(s) before it" in arena.broken_guards()[0]
    with poison.poisoned(0x7F, module=_fake_ops()) as arena:
        assert torch.isfinite(arena.empty(4, dtype=torch.float32)).all() and arena.empty(4, dtype=torch.float32)[0] > 3e38
        assert torch.isnan(arena.empty(4, dtype=torch.float16)).all()
        assert arena.empty(0, dtype=torch.float32).numel() == 0
    assert not arena.broken_guards()


def test_only_empty_is_replaced():
    m = _fake_ops()
    with poison.poisoned(0xFF, module=m) as arena:
        assert m.torch.zeros is torch.zeros and m.torch.float32 is torch.float32 and m.torch.nn is torch.nn
        assert not m.torch.zeros(4).any() and not arena.allocations
        assert m._workspace(X.device, 0) is None
        assert m._workspace(X.device, 100).numel() == 100               # exactly the bytes asked for
    assert m.torch is torch


# ---- coverage of the operator surface ---------------------------------------------------------------------------------
def _reaches_native(path):
    """Public functions of ops.py whose body reaches `_call` / `_topk_reruns` (or calls an mm_* entry point itself), directly or
    through private helpers."""
    with open(path) as f:
        tree = ast.parse(f.read())
    calls = {}
    reach = {"_call", "_topk_reruns"}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            made = [n.func for n in ast.walk(node) if isinstance(n, ast.Call)]
            calls[node.name] = {f.id for f in made if isinstance(f, ast.Name)}
            # an entry point called directly (L.mm_maxsim_fwd_batched(...)); the size queries launch nothing
            if any(isinstance(f, ast.Attribute) and f.attr.startswith("mm_") and not f.attr.endswith("workspace_bytes") for f in made):
                reach.add(node.name)
    grew = True
    while grew:
        grew = False
        for name, callees in calls.items():
            if name not in reach and callees & reach:
                reach.add(name)
                grew = True
    return sorted(n for n in reach if not n.startswith("_"))


def test_every_native_operator_has_a_poisoned_case_or_a_waiver():
    from tests import test_poisoned_memory_gpu as T
    public = _reaches_native(os.path.join(ROOT, "matchmaker_amd", "ops.py"))
    assert len(public) >= 30 and {"maxsim", "maxsim_batched", "maxsim_ragged", "drmm_hist", "dot_topk"} <= set(public), public
    covered = {op for c in T.CASES for op in c.ops}
    for op, reason in T.WAIVERS.items():
        assert op in public and op not in covered, f"waiver for {op}: not an operator, or it has a case"
        assert len(reason.split()) >= 5, f"waiver for {op} gives no reason"
    missing = [op for op in public if op not in covered and op not in T.WAIVERS]
    assert not missing, f"operators of ops.py without a poisoned-memory case or waiver: {missing}"
    assert covered <= set(public), f"cases name operators that ops.py does not have: {sorted(covered - set(public))}"
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names), "duplicate case names"
