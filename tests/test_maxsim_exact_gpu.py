"""GPU: every MaxSim kernel the dispatch can pick, bit for bit against the float64 restatement on the exact-arithmetic cases of
tests/maxsim_exact_cases.py (the forward kernels, the ragged kernel, mm_maxsim_bwd), and the MM_MAXSIM_* A/B twins in child
processes.  There is no tolerance in this file: the inputs make every sum exact in fp32 in any order, so the restatement cast to
the output dtype is the one right answer.  Bits are compared after adding +0.0 to both sides (-0 and +0 compare equal: the pair
backward scales an empty sum by a negative grad_out)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import maxsim_exact_cases as C
from tests import util

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
FORWARD = [r for r in C.TABLE if r[0] != "bwd"]
BACKWARD = [r for r in C.TABLE if r[0] == "bwd"]


def _bits(t):
    t = (t + 0.0).contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_bits(got, ref64, what):
    got = got.cpu()
    exp = torch.from_numpy(np.ascontiguousarray(ref64)).to(torch.float32).to(got.dtype)
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(exp.shape)}"
    differ = _bits(got) != _bits(exp)
    where = differ.nonzero()[:4].tolist()
    assert not differ.any(), (f"{what}: {int(differ.sum())} of {differ.numel()} elements differ in bits, first at {where}: "
                              f"got {[float(got[tuple(w)]) for w in where]}, expected {[float(exp[tuple(w)]) for w in where]}")


def _mask(m, enc, dev):
    m = torch.from_numpy(m)
    if enc == "len":
        n = m.sum(1)
        assert (m == (torch.arange(m.shape[1])[None] < n[:, None])).all(), "lengths encode prefix masks only"
        return n.to(torch.int32).to(dev)
    return m.to({"i64": torch.int64, "u8": torch.uint8, "bool": torch.bool, "f32": torch.float32}[enc]).to(dev)


def _forward(c, dev):
    from matchmaker_amd import ops
    dt = DT[c.dtype]
    q, qm = torch.from_numpy(c.q).to(dt).to(dev), _mask(c.qm, c.enc, dev)
    if c.entry == "ragged":
        return ops.maxsim_ragged(q, torch.from_numpy(c.tokens).to(dt).to(dev), torch.from_numpy(c.begin).to(dev),
                                 torch.from_numpy(c.end).to(dev), qm, pairs_per_query=c.ppq)
    d, dm = torch.from_numpy(c.d).to(dt).to(dev), _mask(c.dm, c.enc, dev)
    if c.entry == "inbatch":
        return ops.maxsim_inbatch(q, qm, d, dm, bug_compatible=c.bug)
    return ops.maxsim(q, d, qm, dm, pairs_per_query=c.ppq)


# --------------------------------------------------------------------------------------------- forward kernels
@pytest.mark.parametrize("row", FORWARD, ids=C.row_name)
def test_forward_scores_are_bit_equal_to_the_float64_restatement(row):
    dev = util.require_gpu()
    c = C.build(*row)
    out = _forward(c, dev)
    assert out.dtype == torch.float32
    _assert_bits(out, C.expect(c), f"{c.name} [{C.expected_kernel(c)}]")


# --------------------------------------------------------------------------------------------- pair backward
def _grad_dtypes(c):
    return [torch.float32] if c.dtype == "f32" else [torch.float32, DT[c.dtype]]


def _bwd_inputs(c, dev, enc=None):
    dt = DT[c.dtype]
    enc = c.enc if enc is None else enc
    return (torch.from_numpy(c.q).to(dt).to(dev), torch.from_numpy(c.d).to(dt).to(dev), _mask(c.qm, enc, dev), _mask(c.dm, enc, dev),
            torch.from_numpy(c.go).float().to(dev))


@pytest.mark.parametrize("row", BACKWARD, ids=C.row_name)
def test_backward_gradients_are_bit_equal_to_the_float64_restatement(row):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    c = C.build(*row)
    ref_q, ref_d = C.expect(c)
    q, d, qm, dm, go = _bwd_inputs(c, dev)
    for gdt in _grad_dtypes(c):
        gq, gd = ops.maxsim_bwd(q, d, qm, dm, go, grad_dtype=gdt)
        assert gq.dtype == gdt and gd.dtype == gdt
        _assert_bits(gq, ref_q, f"{c.name} grad_q {gdt}")
        _assert_bits(gd, ref_d, f"{c.name} grad_d {gdt}")
        gq2, gd2 = ops.maxsim_bwd(q, d, qm, dm, go, grad_dtype=gdt)          # a repeated call: the same bits
        assert torch.equal(_bits(gq), _bits(gq2)) and torch.equal(_bits(gd), _bits(gd2))
        gd = gd.cpu()
        n_dup = 0
        for e in c.edges:                    # two equal rows far apart: the first takes all the gradient, the second exactly none
            if e.kind == "dup":
                n_dup += 1
                assert not _bits(gd[e.doc, e.rows[1]]).any() and gd[e.doc, e.rows[0]].float().abs().sum() > 0, e
            if e.kind == "hole_copy":        # ... and under a hole the later copy takes it
                assert not _bits(gd[e.doc, e.rows[0]]).any() and gd[e.doc, e.rows[1]].float().abs().sum() > 0, e
        assert n_dup or c.D < 7


@pytest.mark.parametrize("row", BACKWARD, ids=C.row_name)
def test_backward_writes_every_byte_of_both_gradients(row):
    """The kernel runs with no memset in front of it: the raw ABI call into NaN-filled buffers leaves no NaN, rows without a
    gradient are zero."""
    from matchmaker_amd import _lib, ops
    dev = util.require_gpu()
    c = C.build(*row)
    L = _lib.lib()
    ref_q, ref_d = C.expect(c)
    q, d, qm, dm, go = _bwd_inputs(c, dev)
    B, Q, E = q.shape
    D = d.shape[1]
    keep_q, qp, qk = ops._mask(qm, B, Q, "q_mask")
    keep_d, dp, dk = ops._mask(dm, B, D, "d_mask")
    for gdt in _grad_dtypes(c):
        gq = torch.full(q.shape, float("nan"), dtype=gdt, device=dev)
        gd = torch.full(d.shape, float("nan"), dtype=gdt, device=dev)
        wsb = L.mm_maxsim_bwd_workspace_bytes(B, Q, D, qk, dk)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        rc = L.mm_maxsim_bwd(q.data_ptr(), d.data_ptr(), qp, qk, dp, dk, go.data_ptr(), gq.data_ptr(), gd.data_ptr(), ops._DT[gdt],
                             B, Q, D, E, ops._DT[q.dtype], ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mm_maxsim_bwd")
        torch.cuda.synchronize()
        assert not torch.isnan(gq).any() and not torch.isnan(gd).any(), "a byte of the gradients was not written"
        _assert_bits(gq, ref_q, f"{c.name} grad_q {gdt}")
        _assert_bits(gd, ref_d, f"{c.name} grad_d {gdt}")
        none_q = torch.from_numpy(~ref_q.any(-1))
        none_d = torch.from_numpy(~ref_d.any(-1))
        assert none_q.any() and none_d.any() and not _bits(gq.cpu()[none_q]).any() and not _bits(gd.cpu()[none_d]).any()


@pytest.mark.parametrize("row", BACKWARD, ids=C.row_name)
def test_backward_gives_the_same_bits_for_every_mask_encoding(row):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    c = C.build(*row)
    ref_q, ref_d = C.expect(c)
    prefix = (c.qm == (np.arange(c.Q)[None] < c.qm.sum(1)[:, None])).all() and (c.dm == (np.arange(c.D)[None] < c.dm.sum(1)[:, None])).all()
    assert prefix == (c.enc == "len") or c.D < 7
    for enc in C.ENCODINGS:
        if enc == c.enc or (enc == "len" and not prefix):
            continue
        q, d, qm, dm, go = _bwd_inputs(c, dev, enc)
        gq, gd = ops.maxsim_bwd(q, d, qm, dm, go, grad_dtype=_grad_dtypes(c)[-1])
        _assert_bits(gq, ref_q, f"{c.name} grad_q with {enc} masks")
        _assert_bits(gd, ref_d, f"{c.name} grad_d with {enc} masks")


# --------------------------------------------------------------------------------------------- the A/B twins
def _switch_cases(switch):
    hits = C.SWITCHES[switch]
    return [c for c in C.cases(("maxsim", "inbatch", "ragged")) if hits is None or C.expected_kernel(c).split(":")[0] in hits]


def _run_switch_cases(switch, path):
    """The child process of test_ab_twin_...: the forward cases `switch` reroutes, outputs into one .npz."""
    name, value = switch.split("=")
    assert os.environ.get(name) == value
    dev = util.require_gpu()
    out = {c.name: _forward(c, dev).cpu().numpy() for c in _switch_cases(switch)}
    np.savez(path, **out)


@pytest.mark.parametrize("switch", list(C.SWITCHES))
def test_ab_twin_is_bit_equal_to_the_float64_restatement(tmp_path, switch):
    """The kernel instantiations behind the MM_MAXSIM_* switches of EnvCfg (mm_internal.h) — the parity twins of performance
    work — on the cases they reroute: one child process with the switch set computes, this process compares with the float64
    expectation (and runs nothing on the GPU for it)."""
    name, value = switch.split("=")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "twin.npz")
    r = subprocess.run([sys.executable, "-c", f"from tests.test_maxsim_exact_gpu import _run_switch_cases; _run_switch_cases({switch!r}, {path!r})"],
                       cwd=root, env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert not os.environ.get(name), "this process must run the default kernels"
    twin = np.load(path)
    want = _switch_cases(switch)
    assert want and set(twin.files) == {c.name for c in want}
    for c in want:
        _assert_bits(torch.from_numpy(twin[c.name]), C.expect(c), f"{switch}: {c.name} [default: {C.expected_kernel(c)}]")
