"""GPU tests of the native contextualiser (matchmaker_amd/contextualize.py over csrc/self_attention.hip).

The kernel through the C ABI: random data against the float64 restatement under the bound of tests/contextualize_reference.py
(4 x the error of torch's own fp32 evaluation + 4 fp32 ulps; 16-bit outputs half a 16-bit ulp more), the bit-exact families of
tests/attention_exact_cases.py in the three dtypes, poisoned memory, determinism, alignment, graph capture and refusals.  Then
the route (`encode`) against eager on the GPU and the restatement, the TK golden, autocast, and the three drop-ins with the
switch on and off.  Every case prints its measured figure before it asserts (pytest -s shows them)."""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from matchmaker_amd import _lib, contextualize, ops
from matchmaker_amd.tk import ECAI20_TK
from matchmaker_amd.tk_sparse import CIKM20_TK_Sparse
from matchmaker_amd.tkl import TKL_sigir20
from oracle import ref_harness as R
from tests import attention_exact_cases as X, contextualize_reference as CR, poison, util

pytestmark = pytest.mark.gpu

LENGTHS = (1, 7, 32, 33, 50, 64, 65, 200, 256)
HEADS = ((10, 30), (8, 48), (2, 32), (1, 64), (3, 8))
SHAPES = [(L, H, dh) for L in LENGTHS for H, dh in HEADS if dh < 64 or L <= 128]
SHAPES16 = [(L, H, dh) for L in (7, 33, 64, 200) for H, dh in ((10, 30), (8, 48))]
LOWP = {torch.float16: np.float16, torch.bfloat16: "bfloat16"}
MU, SIGMA = R.TK_MU, R.TK_SIGMA


def attend(x, mask, H, dev, dtype=torch.float32):
    qkv = torch.from_numpy(np.array(x)).to(dev).to(dtype)
    m = torch.from_numpy(np.array(mask)).to(dev)
    return contextualize.self_attention(qkv, m, H)


def f64(t):
    return t.detach().float().cpu().double().numpy()


def ulp16_size(got, ref, lowp):
    """the 16-bit ulp util.ulps16 measures |got - ref| in"""
    bits = 8 if lowp == "bfloat16" else 11
    mag = np.maximum(np.abs(ref), np.abs(got))
    e = np.floor(np.log2(np.maximum(mag, 2.0 ** (-126 if lowp == "bfloat16" else -14))))
    return 2.0 ** (e - (bits - 1))


# ---- 1. random data against float64, fp32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (1.0, 3.0))
@pytest.mark.parametrize("L,H,dh", SHAPES)
def test_fp32_within_four_times_torchs_own_error(L, H, dh, scale):
    """|got - ref64| <= 4 e_ref + 4 ulp32(|ref64|), e_ref = torch's scaled_dot_product_attention on the CPU with the boolean
    mask against float64 on the same inputs; a sequence with no unmasked key gives exactly +0"""
    dev = util.require_gpu()
    x, mask = CR.random_qkv(L, H, dh, scale)
    ref, bound, e_ref = CR.attention_bound(x, mask, H)
    out = attend(x, mask, H, dev)
    assert out.shape == (5, L, H * dh) and out.dtype == torch.float32
    err = np.abs(f64(out) - ref)
    live = CR.live_rows(mask)
    print(f"self_attention fp32 L={L} H={H} dh={dh} scale={scale}: err {err[live].max():.3e} e_ref {e_ref:.3e} "
          f"ratio {err[live].max() / e_ref if e_ref else float('nan'):.3f}")
    assert not live[4] and not poison.bits(out[4]).any(), "a sequence with no unmasked key is +0 in every row"
    assert (err <= bound).all(), (float((err - bound).max()), e_ref)


# ---- 2. 16-bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
@pytest.mark.parametrize("L,H,dh", SHAPES16)
def test_16_bit_rounds_once_at_the_store(L, H, dh, dtype):
    """the fp32 bound on the 16-bit input values plus half a 16-bit ulp of the result"""
    dev = util.require_gpu()
    x, mask = CR.random_qkv(L, H, dh, 1.0)
    x16 = torch.from_numpy(x.copy()).to(dtype)
    xv = x16.float().numpy()
    ref, bound, e_ref = CR.attention_bound(xv, mask, H)
    out = contextualize.self_attention(x16.to(dev), torch.from_numpy(mask.copy()).to(dev), H)
    assert out.dtype == dtype and out.shape == (5, L, H * dh)
    got = f64(out)
    err = np.abs(got - ref)
    u = ulp16_size(got, ref, LOWP[dtype])
    assert np.allclose(err / u, util.ulps16(got, ref, LOWP[dtype]), rtol=0, atol=1e-9)
    print(f"self_attention {dtype} L={L} H={H} dh={dh}: worst {float((err / u).max()):.3f} ulp16, e_ref {e_ref:.3e}")
    assert not poison.bits(out[4]).any()
    assert (err <= bound + 0.5 * u).all(), float((err - bound - 0.5 * u).max())


# ---- 3. bit-exact families -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16, torch.bfloat16))
@pytest.mark.parametrize("L,H,dh", SHAPES)
def test_exact_families_give_the_stated_bits(L, H, dh, dtype):
    dev = util.require_gpu()
    for family in (X.uniform, X.one_hot):
        qkv, mask, want = family(L, H, dh)[:3]
        out = attend(qkv, mask, H, dev, dtype)
        expect = torch.from_numpy(want).to(torch.float32).to(dtype)      # exact in fp32, rounded once
        diff = poison.bits(out) != poison.bits(expect)
        assert not diff.any(), (family.__name__, int(diff.sum()), [int(v) for v in torch.nonzero(diff)[0]])


@pytest.mark.parametrize("L,H,dh", [(33, 10, 30), (200, 2, 32)])
def test_every_mask_kind_gives_the_same_bits(L, H, dh):
    dev = util.require_gpu()
    x, mask = CR.random_qkv(L, H, dh, 1.0)
    qkv = torch.from_numpy(x.copy()).to(dev)
    m = torch.from_numpy(mask.copy()).to(dev)
    want = contextualize.self_attention(qkv, m, H)
    for other in (m.bool(), m.to(torch.uint8), m.long(), m.double(), m.half()):
        poison.assert_same_bits(want, contextualize.self_attention(qkv, other, H), str(other.dtype))
    prefix = (np.arange(L)[None, :] < np.array([L, L // 2, 1, 0, max(L - 3, 0)])[:, None]).astype(np.float32)
    lens = torch.from_numpy(prefix.sum(1)).to(dev).to(torch.int32)
    poison.assert_same_bits(contextualize.self_attention(qkv, torch.from_numpy(prefix).to(dev), H), contextualize.self_attention(qkv, lens, H), "lengths")
    full = contextualize.self_attention(qkv, None, H)
    poison.assert_same_bits(full, contextualize.self_attention(qkv, torch.ones_like(m), H), "no mask")
    poison.assert_same_bits(full, ops.self_attention(qkv, None, H), "ops forwards")


# ---- 4. poisoned memory ----------------------------------------------------------------------------------------------------------------
POISON = [(33, 10, 30, torch.float32), (200, 8, 48, torch.float16), (65, 3, 8, torch.bfloat16), (1, 1, 64, torch.float32),
          (256, 2, 32, torch.float32)]


@pytest.mark.parametrize("L,H,dh,dtype", POISON)
def test_every_output_element_is_written_and_nothing_else(L, H, dh, dtype):
    dev = util.require_gpu()
    x, mask = CR.random_qkv(L, H, dh, 1.0)
    qkv = torch.from_numpy(x.copy()).to(dev).to(dtype)
    m = torch.from_numpy(mask.copy()).to(dev)
    before = [poison.bits(qkv).clone(), poison.bits(m).clone()]
    fn = lambda: contextualize.self_attention(qkv, m, H)  # noqa: E731
    outs = []
    for p in poison.POISONS:
        out, arena = poison.run(fn, p, module=contextualize, label=f"self_attention {L} {H} {dh} {dtype}")
        assert len(arena.allocations) == 1, "the output came from the arena; there is no workspace"
        outs.append(out)
    poison.assert_same_bits(outs[0], outs[1], f"self_attention {L} {H} {dh} {dtype}")
    poison.assert_same_bits(outs[0], fn(), "against an unpoisoned call")
    assert torch.equal(poison.bits(qkv), before[0]) and torch.equal(poison.bits(m), before[1]), "inputs are untouched"


# ---- 5. determinism, alignment, capture, refusals ---------------------------------------------------------------------------------------
ALIGN = [(33, 10, 30, torch.float32), (200, 8, 48, torch.float16), (64, 2, 32, torch.bfloat16), (50, 3, 8, torch.float32)]


@pytest.mark.parametrize("L,H,dh,dtype", ALIGN)
def test_two_calls_an_offset_view_and_a_captured_replay_give_the_same_bits(L, H, dh, dtype):
    dev = util.require_gpu()
    x, mask = CR.random_qkv(L, H, dh, 1.0)
    qkv = torch.from_numpy(x.copy()).to(dev).to(dtype)
    m = torch.from_numpy(mask.copy()).to(dev)
    want = contextualize.self_attention(qkv, m, H)
    poison.assert_same_bits(want, contextualize.self_attention(qkv, m, H), "two calls")
    big = torch.zeros(qkv.numel() + 9, dtype=dtype, device=dev)
    for off in (1, 2, 4):      # element-aligned, 4- / 8-byte aligned views: narrower loads, the same values
        view = big[off:off + qkv.numel()].view(qkv.shape)
        view.copy_(qkv)
        assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + off * qkv.element_size()
        poison.assert_same_bits(want, contextualize.self_attention(view, m, H), f"a view {off} element(s) into a buffer")
    static, fresh = qkv.clone(), qkv.flip(0).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up off the default stream, as torch.cuda.graph asks
        contextualize.self_attention(static, m, H)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # one launch: no parallel branches
        out = contextualize.self_attention(static, m, H)
    static.copy_(fresh)
    expect = contextualize.self_attention(static, m, H)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    poison.assert_same_bits(expect, out, "captured replay")


def test_unsupported_shapes_raise_and_encode_falls_back():
    dev = util.require_gpu()
    for shape, H, dtype in (((2, 257, 90), 3, torch.float32), ((2, 8, 195), 1, torch.float32), ((2, 8, 186), 2, torch.float16)):
        with pytest.raises(_lib.NativeError) as e:
            contextualize.self_attention(torch.zeros(shape, dtype=dtype, device=dev), None, H)
        assert e.value.code == _lib.MM_EUNSUPPORTED, shape
    with pytest.raises(_lib.NativeError, match="no native backward"):
        contextualize.self_attention(torch.zeros(2, 8, 90, device=dev, requires_grad=True), None, 3)
    for E, H, L in ((130, 2, 9), (60, 2, 257)):      # dh 65; L 257
        enc = make_encoder(E, H, 32, 1).to(dev)
        x = torch.randn(2, L, E, device=dev)
        m = torch.ones(2, L, device=dev)
        assert not contextualize.eligible(enc, x, m)
        with torch.no_grad():
            want = enc(x.transpose(1, 0), src_key_padding_mask=~m.bool()).transpose(1, 0)
            poison.assert_same_bits(want, contextualize.encode(enc, x, m, native=True), "the plain call")


# ---- 6. the route -----------------------------------------------------------------------------------------------------------------------
def make_encoder(E, H, ff, layers, seed=0):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(E, H, dim_feedforward=ff, dropout=0), layers)
    return util.set_deterministic_params(enc).eval().requires_grad_(False)


def route_case(E, L, none_row=True):
    rng = np.random.default_rng([6, E, L])
    x = rng.standard_normal((4, L, E)).astype(np.float32)
    mask = CR.masks(L, ("full", "front", "holes", "none" if none_row else "prefix"))
    return x, mask


ENCODERS = {"tk": (300, 10, 300, 2), "idcm": (384, 8, 384, 1)}


@pytest.mark.parametrize("L", (33, 200))
@pytest.mark.parametrize("name", sorted(ENCODERS))
def test_native_route_against_eager_and_float64(name, L):
    """native within 4 e_eager + 4 ulp32 of float64, e_eager = the eager GPU path's own error on the sequences with a token; the
    sequence without one is compared with the restatement only (eager's backend on the GPU is not pinned)"""
    dev = util.require_gpu()
    E, H, ff, layers = ENCODERS[name]
    cpu = make_encoder(E, H, ff, layers)
    enc = copy.deepcopy(cpu).to(dev)
    x, mask = route_case(E, L)
    ref = CR.encoder64(cpu, x, mask)
    xd, md = torch.from_numpy(x).to(dev), torch.from_numpy(mask).to(dev)
    assert contextualize.eligible(enc, xd, md)
    with torch.no_grad():
        eager = contextualize.encode(enc, xd, md, native=False)
        native = contextualize.encode(enc, xd, md, native=True)
    live = CR.live_rows(mask)
    e_eager = float(np.abs(f64(eager)[live] - ref[live]).max())
    err = np.abs(f64(native) - ref)
    print(f"encode {name} L={L}: native err {err.max():.3e} (live {err[live].max():.3e}) eager err {e_eager:.3e} "
          f"ratio {err[live].max() / e_eager:.3f}")
    assert native.shape == eager.shape == (4, L, E) and torch.isfinite(native).all()
    assert (err <= 4 * e_eager + 4 * CR.ulp32(ref)).all(), float((err - 4 * e_eager - 4 * CR.ulp32(ref)).max())


def test_native_route_replays_the_tk_golden():
    dev = util.require_gpu()
    g = util.load("contextualizer_tk.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ECAI20_TK(300, MU, SIGMA, 10, 2, 300, 200, True, True)
    m = util.set_deterministic_params(m).eval().to(dev)
    contextualize.enable(m)
    for side, pos in (("q", m.positional_features_q), ("d", m.positional_features_d)):
        emb, mask, want = (torch.from_numpy(g[side + k]).to(dev) for k in ("_emb", "_mask", "_out"))
        with torch.no_grad():
            assert contextualize.eligible(m.contextualizer, emb, mask)
            got = m.forward_representation(emb, mask, pos[:, :emb.shape[1], :])
        err = float((got.double() - want.double()).abs().max())
        print(f"TK golden {side}: {err:.3e} (tolerance {CR.golden_tol(g[side + '_out'], 300):.3e})")
        assert err <= CR.golden_tol(g[side + "_out"], 300)


def test_autocast_runs_the_16_bit_kernel(monkeypatch):
    """under torch.autocast(fp16) the linears give a 16-bit projection; native agrees with eager within eager's own error
    against float64 plus 2 fp16 ulps"""
    dev = util.require_gpu()
    E, H, ff, layers = ENCODERS["idcm"]
    cpu = make_encoder(E, H, ff, layers)
    enc = copy.deepcopy(cpu).to(dev)
    x, mask = route_case(E, 64, none_row=False)
    ref = CR.encoder64(cpu, x, mask)
    xd, md = torch.from_numpy(x).to(dev), torch.from_numpy(mask).to(dev)
    seen = []
    real = contextualize.self_attention
    monkeypatch.setattr(contextualize, "self_attention", lambda qkv, m, h: seen.append(qkv.dtype) or real(qkv, m, h))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert contextualize.eligible(enc, xd, md)
        eager = contextualize.encode(enc, xd, md, native=False)
        assert not seen
        native = contextualize.encode(enc, xd, md, native=True)
    assert seen == [torch.float16] * layers and native.dtype == eager.dtype
    e_eager = float(np.abs(f64(eager) - ref).max())
    diff = np.abs(f64(native) - f64(eager))
    u = ulp16_size(f64(native), ref, np.float16)
    print(f"autocast fp16: |native - eager| {diff.max():.3e}, eager err {e_eager:.3e}, native err {np.abs(f64(native) - ref).max():.3e}")
    assert (diff <= e_eager + 2 * u).all()


# ---- 7. the drop-ins -------------------------------------------------------------------------------------------------------------------
def make_model(kind, dev):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind == "tk":
            m = ECAI20_TK(300, MU, SIGMA, 10, 2, 300, 200, True, True)
        elif kind == "tk_sparse":
            m = CIKM20_TK_Sparse(300, MU, SIGMA, 10, 2, 300, 300, 200, True)
        else:
            m = TKL_sigir20(300, MU, SIGMA, 10, 2, 300, 2000, True, True, "embedding")
    util.set_deterministic_params(m.contextualizer)      # the encoder only: TKL keeps mu / sigma as parameters
    return m.eval().to(dev)


def model_inputs(kind, dev):
    B, Q, D = 4, 7, 130 if kind == "tkl" else 33
    rng = np.random.default_rng([7, D])
    qm = (np.arange(Q)[None, :] < np.array([7, 5, 7, 3])[:, None]).astype(np.float32)
    dm = (np.arange(D)[None, :] < np.array([D, D // 2, 9, D - 4])[:, None]).astype(np.float32)
    q = rng.standard_normal((B, Q, 300)).astype(np.float32) * qm[:, :, None]
    d = rng.standard_normal((B, D, 300)).astype(np.float32) * dm[:, :, None]
    return [torch.from_numpy(a).to(dev) for a in (q, d, qm, dm)]


def score_of(out):
    return out[0] if isinstance(out, tuple) else out


@pytest.mark.parametrize("kind", ("tk", "tk_sparse", "tkl"))
def test_drop_in_scores_with_the_switch_off_and_on(kind):
    dev = util.require_gpu()
    m = make_model(kind, dev)
    args = model_inputs(kind, dev)
    with torch.no_grad():
        before = score_of(m(*args)).clone()                 # the instance has not seen the native route
        assert contextualize.enable(m) == 1 and m.native_attention is True
        on = score_of(m(*args)).clone()
        contextualize.enable(m, False)
        off = score_of(m(*args)).clone()
    poison.assert_same_bits(before, off, "native_attention=False")
    err = float((on.double() - off.double()).abs().max())
    print(f"{kind}: |native - eager| scores {err:.3e} (scores up to {float(off.abs().max()):.3f})")
    assert torch.isfinite(on).all() and err <= util.TOL_FP32


@pytest.mark.parametrize("kind", ("tk", "tk_sparse", "tkl"))
def test_training_is_unchanged_by_the_switch(kind):
    dev = util.require_gpu()
    m = make_model(kind, dev).train()
    args = model_inputs(kind, dev)
    runs = []
    for on in (False, True):
        contextualize.enable(m, on)
        m.zero_grad(set_to_none=True)
        score = score_of(m(*args))
        assert score.requires_grad
        score.sum().backward()
        runs.append([score.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None])
    assert len(runs[0]) == len(runs[1]) > 5
    poison.assert_same_bits(runs[0], runs[1], "outputs and gradients in train mode")
