#!/usr/bin/env python
"""Benchmark of the device-side ColBERT store writer (ops.store_append) on one GPU, in one process: one append
per batch of padded encoder output in steady state (HIP events, bench.gpu_time_ms), beside the two paths it replaces.
Prints ONE JSON line:

  calibration   the box's read stream (ops.hbm_stream_probe over 1 GiB) the fractions below are also given against
  legs[]        per shape (512 x 200 x 128 fp16, 512 x 200 x 768 fp16, 2,048 x 200 x 128 bf16; document lengths U{20..200},
                unit token rows, zero padding) and output (the 16-bit rows, or fp8 codes + scales):
                  append_ms       ops.store_append into a resident store (8 input batches rotated, the store refilled from row
                                  0 every 32 appends, so neither side is cache resident by construction)
                  needed_bytes    n_docs * D * E * s read once + the kept bytes written; frac_of_peak / frac_of_calibrated
                  torch_ms        the device-only torch path in the same process: keep = (x != 0).any(-1); rows = x[keep]
                                  (+ ops.fp8_quantize_rows) + a copy into a preallocated store
                  host_ms         the host path it replaces: .cpu().numpy(), the per-document loop of
                                  dense_retrieval.py:237-265 into a numpy block, and the upload of the block (host clock)
                  bit_equal_to_torch_path   the appended rows / codes / scales against the torch path's
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from matchmaker_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
a = ap.parse_args()
dev = torch.device("cuda:0")
SHAPES = [(512, 200, 128, torch.float16), (512, 200, 768, torch.float16), (2048, 200, 128, torch.bfloat16)]
N_IN, REFILL = 8, 32


def make_batch(n_docs, D, E, dtype, g):
    lens = torch.randint(20, D + 1, (n_docs,), generator=g, device=dev)
    x = torch.nn.functional.normalize(torch.randn(n_docs, D, E, generator=g, device=dev), dim=-1).to(dtype)
    x[torch.arange(D, device=dev)[None, :] >= lens[:, None]] = 0
    return x, int(lens.sum())


def host_path(x, block, np_view):
    """dense_retrieval.py:232-265 on one batch, then the upload TokenStore.from_reference_parts does."""
    out = np_view(x.cpu())                                                 # :232
    ins, infos = 0, []
    for i in range(out.shape[0]):                                          # :237-265
        reps = out[i]
        reps = reps[np.abs(reps).sum(-1) > 0, :]
        k = reps.shape[0]
        block[ins: ins + k] = reps
        infos.append((0, ins, ins + k))
        ins += k
    up = torch.from_numpy(block[:ins]).to(dev)
    torch.cuda.synchronize()
    return up


def leg(n_docs, D, E, dtype, fp8, calib_gbs):
    g = torch.Generator(device=dev).manual_seed(77)
    xs, kept = zip(*[make_batch(n_docs, D, E, dtype, g) for _ in range(N_IN)])
    cap = REFILL * max(kept)
    rows = None if fp8 else torch.empty((cap, E), dtype=dtype, device=dev)
    codes = torch.empty((cap, E), dtype=torch.uint8, device=dev) if fp8 else None
    scales = torch.empty((cap,), dtype=torch.float32, device=dev) if fp8 else None
    fill = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    db = torch.empty(n_docs, dtype=torch.int64, device=dev)
    de = torch.empty(n_docs, dtype=torch.int64, device=dev)
    i = [0]

    def append():
        if i[0] % REFILL == 0:
            fill.zero_()
        ops.store_append(xs[i[0] % N_IN], rows, codes, scales, cap, fill, db, de, status)
        i[0] += 1

    t_rows = torch.empty((max(kept), E), dtype=dtype, device=dev) if not fp8 else None
    t_codes = torch.empty((max(kept), E), dtype=torch.uint8, device=dev) if fp8 else None
    t_scales = torch.empty((max(kept),), dtype=torch.float32, device=dev) if fp8 else None
    j = [0]

    def torch_path():
        x = xs[j[0] % N_IN]
        j[0] += 1
        keep = (x != 0).any(-1)
        r = x[keep]
        n = r.shape[0]
        if fp8:
            c, s = ops.fp8_quantize_rows(r)
            t_codes[:n] = c
            t_scales[:n] = s
        else:
            t_rows[:n] = r
        return n

    t_a, t_t = [], []
    for _ in range(2):                                                     # alternated; the first round also warms both
        t_t.append(bench.gpu_time_ms(torch_path, a.steps))
        t_a.append(bench.gpu_time_ms(append, a.steps))
    ms, ms_t = min(t_a), min(t_t)
    assert int(status) == 0
    # the same batch through both, compared
    fill.zero_()
    ops.store_append(xs[0], rows, codes, scales, cap, fill, db, de, status)
    j[0] = 0
    n = torch_path()
    same = int(fill) == n == kept[0]
    if fp8:
        same = same and torch.equal(codes[:n], t_codes[:n]) and torch.equal(scales[:n], t_scales[:n])
    else:
        same = same and torch.equal(rows[:n].view(torch.int16), t_rows[:n].view(torch.int16))
    # the host path (bf16: numpy has no such type, the loop runs on the float32 values and the block holds int16 bits' worth)
    if dtype == torch.bfloat16:
        np_view, block = (lambda t: t.float().numpy()), np.empty((n_docs * D, E), dtype=np.float32)
    else:
        np_view, block = (lambda t: t.numpy()), np.empty((n_docs * D, E), dtype=np.float16)
    host = []
    for r in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_path(xs[r % N_IN], block, np_view)
        host.append(1e3 * (time.perf_counter() - t0))
    s = xs[0].element_size()
    mean_kept = sum(kept) / len(kept)
    need = n_docs * D * E * s + mean_kept * ((E + 4) if fp8 else E * s)
    gbs = need / (ms * 1e-3) / 1e9
    return {"n_docs": n_docs, "D": D, "E": E, "dtype": str(dtype).replace("torch.", ""), "output": "fp8" if fp8 else "16-bit",
            "kept_rows_mean": mean_kept, "append_ms": ms, "torch_ms": ms_t, "host_ms": min(host),
            "host_note": "float32 rows in the loop (numpy has no bfloat16)" if dtype == torch.bfloat16 else None,
            "both_rounds_ms": {"append": t_a, "torch": t_t}, "append_over_torch": ms / ms_t, "needed_bytes": int(need),
            "GBps_needed": gbs, "frac_of_peak": gbs / bench.HBM_PEAK_GBS, "frac_of_calibrated": gbs / calib_gbs,
            "bit_equal_to_torch_path": bool(same)}


probe = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
probe.zero_()
pms = bench.gpu_time_ms(lambda: ops.hbm_stream_probe(probe), a.steps)
calib = (probe.numel() // 8192 * 8192) / (pms * 1e-3) / 1e9
del probe
torch.cuda.empty_cache()
out = {"calibration": {"read_stream_GBps": calib, "ms": pms, "bytes": 1 << 30, "peak_GBps": bench.HBM_PEAK_GBS}, "legs": []}
for n_docs, D, E, dtype in SHAPES:
    for fp8 in (False, True):
        out["legs"].append(leg(n_docs, D, E, dtype, fp8, calib))
        torch.cuda.empty_cache()
print(json.dumps(out))
