#!/usr/bin/env python
"""Benchmark of the native contextualiser route (matchmaker_amd.contextualize over mm_self_attention_fwd) on one
GPU, in one process, on synthetic data.  Each leg alternates the native and the torch form for two rounds; the time is the
median per-call HIP-event interval in steady state (bench.gpu_time_ms).  Prints ONE JSON line:

  core[]     the attention core alone on one q / k / v: contextualize.self_attention on the [B, L, 3E] projection against
             F.scaled_dot_product_attention with the same boolean mask on [B, H, L, dh] views of the same tensor; the kernel's
             rate against the HBM peak on qkv + out bytes and against the fp32 matrix peak on the arithmetic it issues
             (both products on v_mfma_f32_32x32x2_f32 over tiles padded to 32)
  encode[]   contextualize.encode(native=True) against encode(native=False) on the same nn.TransformerEncoder
  tk[]       ECAI20_TK.forward with native_attention on and off (queries [B, 30], documents [B, 200])
  sdpa       the SDPA backends torch had enabled
Shapes: 512 x 200 and 512 x 30 at E 300 / H 10 / ff 300, 2 layers, fp32 (one eval.py batch: documents, queries); 4,096 x 50 on
the same encoder (TKL chunks); 2,048 x 64 at E 384 / H 8 / ff 384, 1 layer, fp16 under autocast (IDCM).  Every leg is printed,
losers included."""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import contextualize  # noqa: E402
from matchmaker_amd.tk import ECAI20_TK  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--small", action="store_true", help="tiny batches (a rehearsal of the script, not a measurement)")
a = ap.parse_args()
dev = torch.device("cuda:0")
HBM_PEAK, F32_MATRIX_PEAK = 8.0e12, 157.3e12
# name: (B, L, E, H, ff, layers, dtype)
SHAPES = {"eval_docs": (512, 200, 300, 10, 300, 2, torch.float32), "eval_queries": (512, 30, 300, 10, 300, 2, torch.float32),
          "tkl_chunks": (4096, 50, 300, 10, 300, 2, torch.float32), "idcm": (2048, 64, 384, 8, 384, 1, torch.float16)}
if a.small:
    SHAPES = {k: (16,) + v[1:] for k, v in SHAPES.items()}
MU, SIGMA = [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9], [0.1] * 11


def timed(steps):
    """{native, torch} -> [round 1 us, round 2 us], alternated (the first round also warms)"""
    out = {True: [], False: []}
    for _ in range(2):
        for native in (True, False):
            out[native].append(1e3 * bench.gpu_time_ms(steps[native], a.steps, timed_ms=40.0, warm_ms=40.0, max_calls=200))
    return {"native_us": out[True], "torch_us": out[False], "torch_over_native": min(out[False]) / min(out[True]),
            "native_faster": max(out[True]) < min(out[False])}


def masks(B, L):
    """document lengths U{L / 10 .. L}, one full row"""
    g = torch.Generator(device=dev).manual_seed(B + L)
    lens = torch.randint(max(1, L // 10), L + 1, (B,), generator=g, device=dev)
    lens[0] = L
    return (torch.arange(L, device=dev)[None, :] < lens[:, None]).float()


def encoder(E, H, ff, layers):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(E, H, dim_feedforward=ff, dropout=0), layers)
    return enc.to(dev).eval().requires_grad_(False)


def core_leg(name):
    B, L, E, H, _, _, dtype = SHAPES[name]
    dh = E // H
    g = torch.Generator(device=dev).manual_seed(L)
    qkv = torch.randn(B, L, 3 * E, generator=g, device=dev).to(dtype)
    m = masks(B, L)
    keep = m.bool()[:, None, None, :].expand(B, 1, L, L)
    q, k, v = (qkv[:, :, i * E:(i + 1) * E].view(B, L, H, dh).transpose(1, 2) for i in range(3))
    r = timed({True: lambda: contextualize.self_attention(qkv, m, H),
               False: lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=keep)})
    t = min(r["native_us"]) * 1e-6
    es = qkv.element_size()
    tiles, dp = -(-L // 32), 32 if dh <= 32 else 64
    hd = (-(-dh // 2) + 7) // 8 * 8
    flop = 2.0 * B * H * (tiles * 32) ** 2 * (2 * hd + dp)      # issued: K Q^T over 2 hd columns, V^T P^T over dp rows
    useful = 4.0 * B * H * L * L * dh
    r.update(name=name, B=B, L=L, E=E, H=H, dtype=str(dtype).replace("torch.", ""),
             hbm_fraction=(qkv.numel() + B * L * E) * es / t / HBM_PEAK, f32_matrix_fraction_issued=flop / t / F32_MATRIX_PEAK,
             f32_matrix_fraction_useful=useful / t / F32_MATRIX_PEAK)
    return r


def encode_leg(name):
    B, L, E, H, ff, layers, dtype = SHAPES[name]
    enc = encoder(E, H, ff, layers)
    x = torch.randn(B, L, E, generator=torch.Generator(device=dev).manual_seed(L), device=dev)
    m = masks(B, L)

    def make(native):
        def step():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16):
                return contextualize.encode(enc, x, m, native=native)
        return step
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16):
        assert contextualize.eligible(enc, x, m)
    return {"name": name, "B": B, "L": L, "E": E, "layers": layers, "dtype": str(dtype).replace("torch.", ""),
            **timed({n: make(n) for n in (True, False)})}


def tk_leg(B):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(0)
        model = ECAI20_TK(300, MU, SIGMA, 10, 2, 300, 200, True, True).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(B)
    qm, dm = masks(B, 30), masks(B, 200)
    q = torch.randn(B, 30, 300, generator=g, device=dev) * qm[:, :, None]
    d = torch.randn(B, 200, 300, generator=g, device=dev) * dm[:, :, None]

    def make(native):
        def step():
            contextualize.enable(model, native)
            with torch.no_grad():
                return model(q, d, qm, dm)
        return step
    return {"name": "ECAI20_TK.forward", "B": B, "Q": 30, "D": 200, **timed({n: make(n) for n in (True, False)})}


core_leg("eval_queries")      # the process's first seconds (clocks, allocator, first launches) belong to no leg
out = {"core": [core_leg(n) for n in SHAPES], "encode": [encode_leg(n) for n in SHAPES], "tk": [tk_leg(16 if a.small else 512)]}
try:
    out["sdpa"] = {"flash": torch.backends.cuda.flash_sdp_enabled(), "mem_efficient": torch.backends.cuda.mem_efficient_sdp_enabled(),
                   "math": torch.backends.cuda.math_sdp_enabled(), "cudnn": torch.backends.cuda.cudnn_sdp_enabled()}
except AttributeError as e:
    out["sdpa"] = {"error": repr(e)}
out["what"] = "us per call, median HIP-event interval in steady state, [round 1, round 2]"
print(json.dumps(out))
