#!/usr/bin/env python
"""Forward + backward of the all-pairs MaxSim (in-batch negatives: colbert.py:154-162, train.py:434-467, 503-524) with the native
backward mm_maxsim_inbatch_bwd, at Q 32 / D 180 / E 128 in bf16 and fp16, 180-token and mixed document lengths:

    32 x 32 (dynamic teacher), 32 x 64 (32 queries, positive + negative documents), 256 x 512 (TAS-Balanced-sized), 1024 x 1024

Yardsticks per leg: the same five torch statements (mm, view / transpose, masked_fill, max, sum) with torch autograd (skipped and
marked when the [Bq Q, Bd D] matrix is too large), mm_maxsim_inbatch_fwd alone, the native backward alone, and — at the two small
shapes — the paired backward mm_maxsim_bwd on Bq Bd replicated pairs plus the two sums it leaves to do.  Needed bytes and FLOP per
forward + backward with their fractions of the HBM and MFMA peaks.

    python tools/bench_inbatch_bwd.py            -> one JSON line

Every leg runs in a child process of its own under `timeout`; the first leg that fails ends the run (nothing more is started on
the GPU after a fault).  Has no part in bench.py.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

Q, D, E = 32, 180, 128
SHAPES = ((32, 32), (32, 64), (256, 512), (1024, 1024))
HBM_PEAK = bench.HBM_PEAK_GBS * 1e9       # B/s
MFMA_PEAK = bench.MFMA_PEAK_16BIT         # FLOP/s, dense bf16 / fp16
EAGER_MAX_BYTES = 4 << 30    # the eager [Bq Q, Bd D] similarity matrix (autograd keeps several copies of it)
LEG_TIMEOUT = 120


def _time(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def leg(Bq, Bd, dtype, lengths):
    import torch
    from matchmaker_amd import ops, torch_ops  # noqa: F401
    dev = torch.device("cuda:0")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(Bq, Q, E, generator=g) * E ** -0.5).to(dt).to(dev)
    d = torch.randn(Bd, D, E, generator=g).to(dt).to(dev)
    go = torch.randn(Bq, Bd, generator=g).to(dev)
    dl = torch.full((Bd,), D) if lengths == "full" else torch.randint(20, D + 1, (Bd,), generator=g)
    qm = torch.ones(Bq, Q, dtype=torch.int64, device=dev)
    dm = (torch.arange(D)[None] < dl[:, None]).long().to(dev)
    iters = 50 if Bq * Bd <= 4096 else (10 if Bq * Bd <= 256 * 512 else 3)
    qg, dg = q.clone().requires_grad_(), d.clone().requires_grad_()

    def native_step():
        qg.grad = dg.grad = None
        torch.ops.mm_native.maxsim_inbatch(qg, qm, dg, dm, False, True, False).backward(go)

    r = {"Bq": Bq, "Bd": Bd, "dtype": dtype, "lengths": lengths, "iters": iters}
    r["native_fwd_bwd_us"] = _time(native_step, iters)
    r["native_fwd_us"] = _time(lambda: ops.maxsim_inbatch(q, qm, d, dm, False, True, False), iters)
    r["native_bwd_us"] = _time(lambda: ops.maxsim_inbatch_bwd(q, qm, d, dm, go, grad_dtype=dt), iters)

    mat = Bq * Q * Bd * D * 2
    if mat <= EAGER_MAX_BYTES:
        keep = dm.bool().unsqueeze(0).unsqueeze(2).expand(Bq, -1, Q, -1)
        qkeep = qm.bool().unsqueeze(1).expand(-1, Bd, -1)

        def eager_step():
            qg.grad = dg.grad = None
            s = torch.mm(qg.reshape(Bq * Q, E), dg.reshape(Bd * D, E).t())
            s = s.view(Bq, Q, Bd, D).transpose(1, 2)
            s = s.masked_fill(~keep, -1000)
            s = s.max(-1).values
            s = s.masked_fill(~qkeep, 0)
            s.sum(-1).backward(go.to(dt))
        r["eager_fwd_bwd_us"] = _time(eager_step, iters)
    else:
        r["eager_fwd_bwd_us"] = None
        r["eager_skipped"] = f"[Bq Q, Bd D] similarity matrix of {mat / 2 ** 30:.1f} GiB (limit {EAGER_MAX_BYTES >> 30} GiB)"

    if Bq * Bd <= 32 * 64:
        qr, dr = q.repeat_interleave(Bd, 0).contiguous(), d.repeat(Bq, 1, 1).contiguous()
        qmr, dmr = qm.repeat_interleave(Bd, 0).contiguous(), dm.repeat(Bq, 1).contiguous()
        gor = go.reshape(-1).contiguous()

        def paired():
            gq, gd = ops.maxsim_bwd(qr, dr, qmr, dmr, gor, grad_dtype=torch.float32)
            return gq.view(Bq, Bd, Q, E).sum(1), gd.view(Bq, Bd, D, E).sum(0)
        r["paired_bwd_replicated_us"] = _time(paired, iters)

    cells = Bq * Bd * Q
    es = 2
    r["needed_bytes"] = (2 * (Bq * Q * E + Bd * D * E) * es          # q and d, read by the forward and by the backward
                         + 2 * Bq * Bd * 4                            # the scores out, grad_out in
                         + (Bq * Q * E + Bd * D * E) * es)            # both gradients out
    r["flop"] = 2 * 2 * Bq * Bd * Q * int(dl.sum().item() / Bd) * E + 2 * 2 * cells * E      # similarities twice + two fma per routed cell
    t = r["native_fwd_bwd_us"] * 1e-6
    r["frac_hbm_peak"] = r["needed_bytes"] / t / HBM_PEAK
    r["frac_mfma_peak"] = r["flop"] / t / MFMA_PEAK
    for k in ("eager_fwd_bwd_us", "paired_bwd_replicated_us"):
        if r.get(k):
            r["native_over_" + k[:-3]] = (r["native_bwd_us"] if k.startswith("paired") else r["native_fwd_bwd_us"]) / r[k]
    r["bwd_over_fwd"] = r["native_bwd_us"] / r["native_fwd_us"]
    return r


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        print("LEG " + json.dumps(leg(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])), flush=True)
        return 0
    legs, failed = [], None
    for Bq, Bd in SHAPES:
        for dtype in ("bf16", "fp16"):
            for lengths in ("full", "mixed"):
                cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), "--leg", str(Bq), str(Bd),
                       dtype, lengths]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                line = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
                if p.returncode != 0 or not line:
                    failed = {"leg": cmd[-4:], "returncode": p.returncode, "stderr_tail": p.stderr[-400:]}
                    break
                legs.append(json.loads(line[-1][4:]))
            if failed:
                break
        if failed:
            break
    print(json.dumps({"bench": "maxsim_inbatch_fwd_bwd", "Q": Q, "D": D, "E": E, "hbm_peak_Bps": HBM_PEAK, "mfma_peak_flops": MFMA_PEAK,
                      "legs": legs, "failed": failed}))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
